"""Feature-map driver — the counterpart of the reference's ``generate_feature_map.py`` (flags ``:22-32``, loop ``:179-265``) over
this project's loader and dump format: runs ``DAVO.inference(mode='feature')`` with ``enable_feature_mode(features='heat')`` over a
sequence, so that per window two [H,W] planes and two scalars per head leave the GPU instead of the two resized cnv6 maps.

    python -m davo_amd.generate_feature_map --test_seq 9 --concat_img_dir DUMP --ckpt_file W.npz --output_dir out --version v1-...
    python -m davo_amd.generate_feature_map --synthetic 7 --output_dir out          # seeded synthetic inputs and weights

Written under ``--output_dir`` (NN = the sequence, FFFFFF = the window's target frame, ``tgt_idx - max_src_offset + 1``):

    NN-tgtsrc0.txt, NN-tgtsrc1.txt        the attention tables (``:152-155,187-192``): a title line, then per window
                                          ``"%06d,%s\\n"`` with the 19 values of att_19[1] (src0) / att_19[2] (src1)
    NN-featuremaps/FFFFFF-{rot,trans}_feature-{avg,sum}.png
                                          the 8-bit index images ``color_map`` computes before its colour lookup (``:208-214``):
                                          (plane / maximum * 255).astype(uint8) with plane = mean over the channels and maximum =
                                          the map's max() for ``avg``, plane = sum over the channels and maximum = plane.max()
                                          for ``sum`` (``:249-263``); all zeros where the maximum is 0
    NN-featuremaps/FFFFFF-{rot,trans}_feature-{avg,sum}.npy      with ``--npy``: the float32 planes themselves
    NN-pred_kitti_pose.txt                the trajectory, as run_kitti_pose writes it (``:158,383-421``)

Not built: the JET lookup (cv2.applyColorMap), the overlays on the frames (cv2.addWeighted) and the merged figures need cv2,
which this project does not depend on; the index images are what those colourings are functions of.  The reference's hard-coded
per-sequence window filter (``:194-203``) is not kept either: every window is written."""
import argparse
import os

import numpy as np

from . import sequence as S
from .davo import DAVO
from .version import FLAGSHIP_VERSION

# the 19 Cityscapes train classes in train-id order: the title line of the attention tables
SEG_LABELS = ("road", "sidewalk", "building", "wall", "fence", "pole", "traffic light", "traffic sign", "vegetation", "terrain",
              "sky", "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")
HEADS = ("rot", "trans")
KINDS = ("avg", "sum")


def index_image(plane, maximum):
    """``color_map``'s 8-bit image before the colour lookup (generate_feature_map.py:208-214): (plane / maximum * 255) in
    float32, truncated to uint8; all zeros where maximum is 0 (the reference divides by zero there)."""
    plane = np.asarray(plane, np.float32)
    maximum = np.float32(maximum)
    if not maximum > 0:
        return np.zeros(plane.shape, np.uint8)
    return (plane / maximum * 255).astype(np.uint8)


def frame_id(window):
    """window w has target frame w + 1 = the reference's ``tgt_idx - max_src_offset + 1`` (seq_length 3)."""
    return window + 1


def feature_file(window, head, kind, ext="png"):
    """'%.6d-{rot,trans}_feature-{avg,sum}.png' (generate_feature_map.py:251-265)"""
    if head not in HEADS or kind not in KINDS:
        raise ValueError("head %r / kind %r: choose from %s / %s" % (head, kind, HEADS, KINDS))
    return "%.6d-%s_feature-%s.%s" % (frame_id(window), head, kind, ext)


def table_title():
    return "id,%s\n" % ",".join(SEG_LABELS)                                   # :154-155


def table_line(window, row):
    """one attention-table line (generate_feature_map.py:191-192): the frame id, then str() of each of the 19 values"""
    row = np.asarray(row, np.float32).reshape(-1)
    if row.size != len(SEG_LABELS):
        raise ValueError("an attention row has %d values, got %d" % (len(SEG_LABELS), row.size))
    return "%06d,%s\n" % (frame_id(window), ",".join(str(v) for v in row))


def window_images(features, j):
    """{(head, kind): (float32 plane, uint8 index image)} of window j of a features='heat' dict's 'features'"""
    out = {}
    for head in HEADS:
        total, mean, top = features[head + "_sum"][j], features[head + "_avg"][j], features[head + "_max"][j]
        out[head, "avg"] = (mean, index_image(mean, top))                     # :249,260
        out[head, "sum"] = (total, index_image(total, total.max()))           # :252,263
    return out


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_size", type=int, default=1)                      # generate_feature_map.py:23-31
    ap.add_argument("--img_height", type=int, default=128)
    ap.add_argument("--img_width", type=int, default=416)
    ap.add_argument("--seq_length", type=int, default=3)
    ap.add_argument("--test_seq", type=int, default=9)
    ap.add_argument("--concat_img_dir", default=None)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--ckpt_file", default=None)
    ap.add_argument("--version", default=FLAGSHIP_VERSION)
    ap.add_argument("--synthetic", type=int, default=None, help="frame count of a synthetic sequence (seeded inputs and weights)")
    ap.add_argument("--npy", action="store_true", help="also write the float32 planes beside the index images")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--labels", choices=("f32", "u8"), default="f32",
                    help="u8: the label maps are loaded and handed to the library as uint8 class ids (davo_set_label_format); "
                         "the written files are the same")
    ap.add_argument("--depth", choices=("f32", "f16"), default="f32",
                    help="f16: the depth planes of a depth-source version are handed over as IEEE binary16 (include/davo_hip.h: "
                         "davo_set_depth_format; float32 -monodepth2_depth.npy files are rounded by davo_amd.depth_to_f16, float16 ones "
                         "read as they are).  The files written are those of a float32 run on the rounded planes")
    ap.add_argument("--flip", action="store_true",
                    help="run the left-right mirrored sequence (include/davo_hip.h: davo_set_flip, each frame mirrored on its own); the "
                         "files go under <output_dir>-flip, as the reference's flip switch appends `-flip' to its output root "
                         "(generate_feature_map.py:118-129)")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.seq_length != 3:
        ap.error("--seq_length %d: the pose path is built for 3-frame windows" % a.seq_length)
    if a.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    from PIL import Image
    from .version import parse_version
    H, W, seq = a.img_height, a.img_width, a.test_seq
    cfg = parse_version(a.version)
    if cfg.att_source == "se_flow_depthseg_sep":
        # the table files hold att_19[1] / att_19[2], one 19-value row per window; this branch applies two tables per frame, chosen
        # per pixel by depth, and sets no att_19s (reference davo.py:1470; its own script fails on line 187 there)
        raise SystemExit("davo_amd.generate_feature_map: version `%s': `-se_flow_on_depthseg_seplayers' has no per-frame 19-class "
                         "table to write (a near and a far table are selected per pixel by depth); use "
                         "DAVO.inference(mode='feature') for its attention maps and features" % a.version)
    synthetic = bool(a.synthetic)
    depth_arg = ("f16" if a.depth == "f16" else True) if cfg.needs_depth else False      # the loaders' ``depth`` argument
    if synthetic:
        from . import synth
        n_frames = a.synthetic
        load = S.synthetic_window_loader(H, W, depth=depth_arg, labels=a.labels)
        weights = synth.make_weights(a.version)
    else:
        if not a.concat_img_dir or not a.ckpt_file:
            ap.error("--concat_img_dir and --ckpt_file (or --synthetic N) are required")
        d = os.path.join(a.concat_img_dir, "%.2d" % seq)
        if not os.path.isdir(d):
            raise SystemExit("davo_amd.generate_feature_map: sequence %.2d: no directory %s" % (seq, d))
        n_frames = sum(1 for f in os.listdir(d) if f.endswith(".jpg")) + 2 * int((a.seq_length - 1) / 2)       # :83-84
        from .tf_checkpoint import load_weights
        load = S.kitti_window_loader(a.concat_img_dir, seq, n_frames, H, W, depth=depth_arg, seg_planes=(0, 1, 2), labels=a.labels)
        weights = load_weights(a.ckpt_file)
    if n_frames < 3:
        raise SystemExit("davo_amd.generate_feature_map: sequence %.2d has %d frames: a window needs three" % (seq, n_frames))
    n_windows = n_frames - 2
    if a.flip:
        a.output_dir = a.output_dir.rstrip("/" + os.sep) + "-flip"
    map_dir = os.path.join(a.output_dir, "%.2d-featuremaps" % seq)
    os.makedirs(map_dir, exist_ok=True)
    system = DAVO(version=a.version, device=a.device, flip=a.flip).enable_feature_mode(features='heat')
    if a.labels == "u8":
        system.use_u8_labels()
    if a.depth == "f16":
        system.use_f16_depth()
    system.setup_inference(H, W, "davo", a.seq_length, a.batch_size)
    system.load_weights(weights)
    poses = np.empty((n_windows, 2, 6), np.float32)
    try:
        with open(os.path.join(a.output_dir, "%.2d-tgtsrc0.txt" % seq), "w") as f0, \
                open(os.path.join(a.output_dir, "%.2d-tgtsrc1.txt" % seq), "w") as f1:
            f0.write(table_title())
            f1.write(table_title())
            for s in range(0, n_windows, a.batch_size):
                e = min(s + a.batch_size, n_windows)
                pred = system.inference(None, mode='feature', inputs=load(s, e))
                poses[s:e] = pred['pose']
                att_19 = pred['masks']['att_19']                              # tgt, src0, src1: [B,1,1,19] each
                for j in range(e - s):
                    w = s + j
                    f0.write(table_line(w, att_19[1][j, 0, 0]))
                    f1.write(table_line(w, att_19[2][j, 0, 0]))
                    for (head, kind), (plane, image) in window_images(pred['features'], j).items():
                        Image.fromarray(image).save(os.path.join(map_dir, feature_file(w, head, kind)))
                        if a.npy:
                            np.save(os.path.join(map_dir, feature_file(w, head, kind, "npy")), plane)
    finally:
        system.engine.close()
    out = os.path.join(a.output_dir, "%.2d-pred_kitti_pose.txt" % seq)
    S.write_kitti_poses(out, S.stitch_trajectory(poses))
    print("Done. Please check %s and %s" % (map_dir, out))


if __name__ == "__main__":
    main()

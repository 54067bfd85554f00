"""What the feature export costs ("Feature export"): wall time of Engine.forward_features against
Engine.forward on the same inputs, in alternating rounds in one process, and - with --profile - a short run of feature calls
alone for `rocprofv3 --kernel-trace --stats -- python tools/feature_export_measure.py --profile ...`.

    python tools/feature_export_measure.py [--batch 8] [--height 128] [--width 416] [--rounds 5] [--calls 10]

One JSON line per precision: median wall time of one call of each kind, of forward_features with only the two feature maps, only
the maps, and nothing wanted (a plain forward through the new entry point), and the bytes an export delivers."""
import argparse
import json
import statistics
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from davo_amd import Engine, FLAGSHIP_VERSION, parse_version, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--precision", choices=["f16x3", "f32", "both"], default="both")
    ap.add_argument("--profile", action="store_true", help="feature calls only, a few of them: the run rocprofv3 wraps")
    a = ap.parse_args()
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = a.batch, a.height, a.width
    img, flow, seg = synth.make_inputs(B, H, W)
    weights = synth.make_weights(cfg)
    kinds = {"forward": None, "features_all": Engine.FEATURE_OUTPUTS, "features_resize_only": ("feat_rot", "feat_trans"),
             "features_maps_only": ("att_19", "attention", "masked_image", "image"), "features_none": ()}
    for precision in (["f16x3", "f32"] if a.precision == "both" else [a.precision]):
        e = Engine(cfg, H, W, B)
        e.load_weights(weights)
        e.set_precision(precision)
        e.set_feature_export(True)

        def call(kind):
            t0 = time.perf_counter()
            if kinds[kind] is None:
                e.forward(img, flow, seg)
            else:
                e.forward_features(img, flow, seg, want=kinds[kind])
            return (time.perf_counter() - t0) * 1e3

        for kind in kinds:                      # warm-up: weights packed, workspaces and staging allocated
            call(kind)
        if a.profile:
            for _ in range(a.calls):
                call("features_all")
            e.close()
            continue
        samples = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for kind in kinds:
                samples[kind] += [call(kind) for _ in range(a.calls)]
        c6 = cfg.cnv6_out
        out = {"precision": precision, "B": B, "H": H, "W": W, "rounds": a.rounds, "calls_per_round": a.calls,
               "median_ms": {k: round(statistics.median(v), 3) for k, v in samples.items()},
               "min_ms": {k: round(min(v), 3) for k, v in samples.items()},
               "feature_bytes": 2 * B * H * W * c6 * 4, "map_bytes": B * (3 * 19 + 3 * H * W * 7) * 4}
        print(json.dumps(out), flush=True)
        e.close()


if __name__ == "__main__":
    main()

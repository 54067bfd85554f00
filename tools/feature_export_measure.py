"""What the feature export costs ("Feature export"): wall time of Engine.forward_features against
Engine.forward on the same inputs, in alternating rounds in one process, and - with --profile - a short run of feature calls
alone for `rocprofv3 --kernel-trace --stats -- python tools/feature_export_measure.py --profile ...`.

    python tools/feature_export_measure.py [--batch 8] [--height 128] [--width 416] [--rounds 5] [--calls 10]

One JSON line per precision: median wall time of one call of each kind, of forward_features with only the two feature maps, only
the maps, and nothing wanted (a plain forward through the new entry point), and the bytes an export delivers.

    python tools/feature_export_measure.py --heat [--calls 20] [--step-timeout 120]

The heat arm (davo_forward_heat against davo_forward_features): at the flagship shape, B = 1 and B = 8, one step each for
davo_forward, davo_forward_features with both full maps and davo_forward_heat with all four heat members.  Every step is a child
process of its own under its own time limit; the first step that fails or runs out of time ends the run, nothing is started after
it.  One JSON line per step, then one with the heat / full ratio per batch size."""
import argparse
import json
import statistics
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from davo_amd import Engine, FLAGSHIP_VERSION, parse_version, synth  # noqa: E402


HEAT_STEPS = ("forward", "features_full", "heat")


def heat_step(kind, B, H, W, calls, precision):
    """one step of the heat arm, in this process: -> its JSON record"""
    cfg = parse_version(FLAGSHIP_VERSION)
    img, flow, seg = synth.make_inputs(B, H, W)
    e = Engine(cfg, H, W, B)
    e.load_weights(synth.make_weights(cfg))
    e.set_precision(precision)
    c6 = cfg.cnv6_out
    if kind == "features_full":
        e.set_feature_export(True)
        run, copied = (lambda: e.forward_features(img, flow, seg, want=("feat_rot", "feat_trans"))), 2 * B * H * W * c6 * 4
    elif kind == "heat":
        e.set_heat_export(True)
        run, copied = (lambda: e.forward_features(img, flow, seg, want=Engine.HEAT_OUTPUTS)), 2 * B * (H * W + 1) * 4
    else:
        run, copied = (lambda: e.forward(img, flow, seg)), 0
    for _ in range(3):                         # warm-up: weights packed, workspaces and staging allocated
        run()
    samples = []
    for _ in range(calls):
        t0 = time.perf_counter()
        run()
        samples.append((time.perf_counter() - t0) * 1e3)
    e.close()
    return {"step": kind, "precision": precision, "B": B, "H": H, "W": W, "calls": calls, "median_ms": round(statistics.median(samples), 3),
            "min_ms": round(min(samples), 3), "export_bytes_copied": copied + B * 12 * 4}


def heat_arm(a):
    """the parent of the heat arm: starts the steps one after the other, each under its own time limit, and never touches the GPU"""
    import subprocess
    results = {}
    for B in (1, 8):
        for kind in HEAT_STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--heat-step", kind, "--batch", str(B), "--height", str(a.height),
                   "--width", str(a.width), "--calls", str(a.calls), "--precision", "f16x3" if a.precision == "both" else a.precision]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit("step %s B=%d ran past %d s: stopped, nothing started after it" % (kind, B, a.step_timeout))
            if out.returncode != 0:
                raise SystemExit("step %s B=%d failed with status %d: stopped, nothing started after it\n%s" % (kind, B, out.returncode, out.stderr[-2000:]))
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            results[B, kind] = rec
    print(json.dumps({"heat_over_full_median": {str(B): round(results[B, "heat"]["median_ms"] / results[B, "features_full"]["median_ms"], 4) for B in (1, 8)},
                      "heat_over_forward_median": {str(B): round(results[B, "heat"]["median_ms"] / results[B, "forward"]["median_ms"], 4) for B in (1, 8)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heat", action="store_true", help="the heat arm: forward / full maps / heat at B = 1 and 8, a child process per step")
    ap.add_argument("--heat-step", choices=HEAT_STEPS, default=None, help="(the heat arm's child) run this one step in this process")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a step of the heat arm may take")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--precision", choices=["f16x3", "f32", "both"], default="both")
    ap.add_argument("--profile", action="store_true", help="feature calls only, a few of them: the run rocprofv3 wraps")
    a = ap.parse_args()
    if a.heat:
        return heat_arm(a)
    if a.heat_step:
        print(json.dumps(heat_step(a.heat_step, a.batch, a.height, a.width, a.calls, "f16x3" if a.precision == "both" else a.precision)), flush=True)
        return
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

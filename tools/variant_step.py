"""Step time of any runnable variant on one GPU (bench.py measures the flagship only): synthetic inputs resident in HBM,
`--warmup` untimed then `--steps` timed davo_forward_device calls, one JSON line per version.  Versions are run in
alternating rounds (`--rounds`) so that a drift of the card's clocks does not favour one of them.

    python tools/variant_step.py --precision f16x3 --batch 32 <version> [<version> ...]

`--pairs ARM [ARM ...]` runs every version once per arm, the arms alternating inside each round: ARM is a pair selection
(both | src0 | src1; include/davo_hip.h: davo_set_pairs), optionally `@B` for that arm's batch size.  The measurement of
DESIGN.md section 2 - does one pair of B windows run the launches of both pairs of B / 2? - is

    python tools/variant_step.py --batch 32 --rounds 5 --pairs both src1 both@16 <version>

`--stages N` adds the library's own event profile (Engine.profile(1)) behind the timed rounds: N forwards per version and round,
the versions taken in forward order in even rounds and in reverse order in odd ones, so that whatever the card's clocks do while
events bracket every launch falls on each version alike; the line then carries `stage_us` (mean us per launch and profile entry
over the rounds) and `stage_us_per_round`.  The measurement of DESIGN.md section 2, "Depth-split flow attention", is

    python tools/variant_step.py --precision f16x3 --batch 32 --rounds 6 --stages 20 <flagship> <-se_flow_on_depthseg_seplayers string>

`--flip ARM [ARM ...]` (off | on; include/davo_hip.h: davo_set_flip) multiplies the arms by the mirror setting, and `--layout
frames` issues davo_forward_device_frames on a synthetic frame sequence instead of davo_forward_device on windows.  What the
mirror costs on resident inputs in either layout ("Mirrored inputs") is

    python tools/variant_step.py --batch 32 --rounds 5 --stages 20 --flip off on [--layout frames] <flagship>

`--depth ARM [ARM ...]` (f32 | f16; include/davo_hip.h: davo_set_depth_format) multiplies the arms by the depth format: the f16
arm's engine takes davo_amd.depth_to_f16 of the same planes.  Both formats of a depth source in one process, alternating
("Depth planes as binary16"):

    python tools/variant_step.py --batch 32 --rounds 6 --stages 20 <a depth-source version> --depth f32 f16

Under `rocprofv3 --kernel-trace --stats -- python3 tools/variant_step.py ...` it gives the per-kernel table of a variant."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from davo_amd import Engine, synth, parse_version, depth_to_f16  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("versions", nargs="+")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--precision", choices=["f16x3", "f32"], default="f16x3")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--pairs", nargs="+", default=None, metavar="ARM",
                    help="arms of (pair selection[@batch]): both | src0 | src1, e.g. --pairs both src1 both@16")
    ap.add_argument("--stages", type=int, default=0, metavar="N",
                    help="after the timed rounds, profile N forwards per version and round (alternating order): us per launch and profile entry")
    ap.add_argument("--flip", nargs="+", default=None, choices=["off", "on"], metavar="ARM",
                    help="arms of the mirror setting (davo_set_flip): off | on, e.g. --flip off on; every pair arm runs once per flip arm")
    ap.add_argument("--layout", choices=["windows", "frames"], default="windows",
                    help="windows: davo_forward_device; frames: davo_forward_device_frames (the timed step includes the gather)")
    ap.add_argument("--depth", nargs="+", default=None, choices=["f32", "f16"], metavar="ARM",
                    help="arms of the depth format (davo_set_depth_format): f32 | f16, e.g. --depth f32 f16; every other arm runs once per depth arm")
    a = ap.parse_args()
    H, W = a.height, a.width
    arms = []
    for arm in a.pairs or ["both"]:
        sel, _, b = arm.partition("@")
        if sel not in Engine.PAIRS or (b and not b.isdigit()):
            ap.error("--pairs: `%s' is not both | src0 | src1, optionally @batch" % arm)
        arms += [(sel, int(b) if b else a.batch, flip == "on", dfmt) for flip in (a.flip or ["off"]) for dfmt in (a.depth or ["f32"])]
    Bmax = max(arm[1] for arm in arms)
    frames = synth.make_frames(Bmax + 2, H, W, depth=True) if a.layout == "frames" else None
    img, flow, seg = synth.make_inputs(Bmax, H, W)
    depth = synth.make_depth(Bmax, H, W)           # uploaded for the depth sources only
    runs = []
    for v in a.versions:
        cfg = parse_version(v)
        for sel, B, flip, dfmt in arms:
            e = Engine(cfg, H, W, B, depth=dfmt)
            e.load_weights(synth.make_weights(cfg))
            e.set_precision(a.precision)
            e.set_pairs(sel)
            e.set_flip(flip)
            if frames is not None:
                parts, dep = (frames[0][:B + 2], frames[1][:B], frames[2][:B + 2]), frames[3][:B + 2]
                e.step = e.forward_device_frames
            else:
                parts, dep = (img[:B], flow[:B], seg[:B]), depth[:B]
                e.step = e.forward_device
            bufs = [e.alloc(x.nbytes).upload(x) for x in parts] + [e.alloc(B * 12 * 4)]
            dep = depth_to_f16(dep) if dfmt == "f16" else dep
            kw = {"depth": e.alloc(dep.nbytes).upload(dep)} if cfg.needs_depth else {}
            for _ in range(a.warmup):
                e.step(B, *bufs, **kw)
            e.synchronize()
            runs.append((v, e, bufs, [], kw, sel, B))
    for _ in range(a.rounds):
        for v, e, bufs, ms, kw, sel, B in runs:
            e.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                e.step(B, *bufs, **kw)
            e.synchronize()
            ms.append((time.perf_counter() - t) * 1e3 / a.steps)
    stages = [[] for _ in runs]                     # per run: one {entry: us per launch} per round
    for rnd in range(a.rounds if a.stages > 0 else 0):
        order = list(range(len(runs)))
        for i in (order if rnd % 2 == 0 else order[::-1]):
            v, e, bufs, ms, kw, sel, B = runs[i]
            e.profile(1)
            e.profile_reset()
            for _ in range(a.stages):
                e.step(B, *bufs, **kw)
            e.synchronize()
            stages[i].append({k: 1e3 * total / n for k, (n, total) in e.profile_entries().items() if n > 0})
            e.profile(0)
    for (v, e, bufs, ms, kw, sel, B), st in zip(runs, stages):
        bufs = bufs + list(kw.values())
        pose = bufs[3].download((B, 2, 6))
        best = min(ms)
        line = {"version": v, "precision": a.precision, "batch": B, "height": H, "width": W, "steps": a.steps,
                "ms_per_step": round(best, 4), "ms_per_round": [round(x, 4) for x in ms],
                "triplets_per_s": round(B / best * 1e3, 1), "finite": bool(np.isfinite(pose).all())}
        if st:
            line.update(stage_us={k: round(sum(r[k] for r in st) / len(st), 2) for k in st[0]},
                        stage_us_per_round=[{k: round(x, 2) for k, x in r.items()} for r in st])
        if a.pairs:
            line.update(pairs=sel, plan=[e.last_plan(l) for l in range(7)])
        if a.depth:
            line.update(depth=e.depth)
        if a.flip or a.layout != "windows":
            line.update(flip=e.flip, layout=a.layout)
        print(json.dumps(line), flush=True)
        for buf in bufs:
            buf.free()
        e.close()


if __name__ == "__main__":
    main()

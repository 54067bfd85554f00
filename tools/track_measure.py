#!/usr/bin/env python
"""Online tracking against what a live caller does today ("Online tracking"): measured, not gated.

One process on one MI355X, 128x416, flagship, f16x3, byte labels and binary16 flow, page-locked host arrays; the arms alternate
inside every round (round 0 warms up) and every figure comes with the spread between the repeats of its own arm.

  latency     S = 1: wall time per frame from the push to the delivered pose - `track` = davo_track_push + davo_wait(0) under the
              trajectory policy against `frames` = davo_submit_frames(N = 1) + davo_wait(0) under DAVO_PAIRS_SRC1 on a three-frame
              array the caller keeps (the existing code); with 1 and 4 in-flight slots
  throughput  S = 32: windows/s of 32 lanes per push against davo_submit_frames(N = 32) under DAVO_PAIRS_SRC1, three slots,
              pushes streamed (hold = 8: the arrays are never recycled)

    python tools/track_measure.py --out profiles/track_measure.jsonl [--rounds 5] [--frames 400]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                                     # noqa: E402
from davo_amd import Engine, FLAGSHIP_VERSION, parse_version, pinned_empty, synth     # noqa: E402
from davo_amd.frames import frames_plan, track_plan                                    # noqa: E402

H, W = 128, 416
FMT = dict(labels="u8", flow="f16")


def pinned(a):
    d = pinned_empty(a.shape, a.dtype)
    d[...] = a
    return d


M = 8                                                     # distinct pushes, cycled: the arithmetic does not depend on the values' variety


def lanes_of(S):
    """S lanes x M pushes, stacked per push: frames [M,S,H,W,3], flow2 [M,S,2,H,W,2], seg [M,S,H,W,1] (one draw, repeated over
    the lanes)"""
    fr, fl, sg = synth.make_frames(M + 2, H, W, **FMT)
    fr, sg = fr[:M], sg[:M]
    rep = lambda a: pinned(np.repeat(a[:, None], S, axis=1))      # noqa: E731
    return rep(fr), rep(fl), rep(sg)


def latency(e, rounds, n):
    """-> {arm: [us per frame, one figure per round]}"""
    fr, fl, sg = lanes_of(1)
    out = np.empty((1, 2, 6), np.float32)
    three = [pinned(np.zeros((3,) + a.shape[2:], a.dtype)) for a in (fr, sg)]       # the caller's own last three frames
    res = {"track": [], "frames": []}
    for r in range(rounds + 1):
        for arm in ("track", "frames"):
            if arm == "track":
                e.track_begin(1, "trajectory")
                e.track_push(fr[0], None, sg[0], None)
                e.track_push(fr[1], None, sg[1], None)
                t0 = time.perf_counter()
                for t in range(2, n):
                    e.track_push(fr[t % M], fl[t % M], sg[t % M], out)
                    e.wait(0)
                dt = time.perf_counter() - t0
                e.track_end()
            else:
                e.set_pairs("src1")
                for k in range(2):
                    three[0][k + 1], three[1][k + 1] = fr[k, 0], sg[k, 0]
                t0 = time.perf_counter()
                for t in range(2, n):
                    for buf, src in zip(three, (fr, sg)):          # what the caller does today: keep two frames, rebuild three
                        buf[0], buf[1], buf[2] = buf[1], buf[2], src[t % M, 0]
                    e.submit_frames(three[0], fl[t % M], three[1], out)
                    e.wait(0)
                dt = time.perf_counter() - t0
            if r:
                res[arm].append(dt / (n - 2) * 1e6)
    return res


def throughput(e, rounds, n, S):
    """-> {arm: [windows/s, one figure per round]}"""
    fr, fl, sg = lanes_of(S)
    # the frame layout's batch of S windows: S + 2 consecutive frames of ONE video - as many windows per call, the existing code
    f2 = tuple(pinned(a) for a in synth.make_frames(S + 2, H, W, **FMT))
    outs = [np.empty((S, 2, 6), np.float32) for _ in range(n)]
    res = {"track": [], "frames": []}
    for r in range(rounds + 1):
        for arm in ("track", "frames"):
            if arm == "track":
                e.track_begin(S, "trajectory")
                e.track_push(fr[0], None, sg[0], None)
                e.track_push(fr[1], None, sg[1], None)
                e.track_push(fr[2], fl[2], sg[2], outs[2], hold=8)      # the session's one both-pairs window: outside the clock
                e.wait()
                t0 = time.perf_counter()
                for t in range(3, n):
                    e.track_push(fr[t % M], fl[t % M], sg[t % M], outs[t], hold=8)
                e.wait()
                dt = time.perf_counter() - t0
                e.track_end()
            else:
                e.set_pairs("src1")
                t0 = time.perf_counter()
                for t in range(3, n):
                    e.submit_frames(*f2, outs[t], hold=8)
                e.wait()
                dt = time.perf_counter() - t0
            if r:
                res[arm].append(S * (n - 3) / dt)
    return res


def summary(vals):
    v = sorted(vals)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "rounds": vals}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=400)
    a = ap.parse_args()
    cfg = parse_version(FLAGSHIP_VERSION)
    weights = synth.make_weights(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rows = []
    for inflight in (1, 4):
        e = Engine(cfg, H, W, 1, **FMT)
        e.load_weights(weights)
        e.set_inflight(inflight)
        res = latency(e, a.rounds, a.frames)
        e.close()
        rows.append({"measure": "latency_us_per_frame", "lanes": 1, "inflight": inflight,
                     "link_bytes": {"track": track_plan(H, W, 1, "src1", **FMT), "frames": frames_plan(H, W, 1, "src1", **FMT)["link_bytes"]},
                     **{arm: summary(v) for arm, v in res.items()}})
    S = 32
    e = Engine(cfg, H, W, S, **FMT)
    e.load_weights(weights)
    e.set_inflight(3)
    res = throughput(e, a.rounds, 60, S)
    e.close()
    rows.append({"measure": "throughput_windows_per_s", "lanes": S, "inflight": 3,
                 "link_bytes": {"track": track_plan(H, W, S, "src1", **FMT), "frames": frames_plan(H, W, S, "src1", **FMT)["link_bytes"]},
                 **{arm: summary(v) for arm, v in res.items()}})
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
            print(json.dumps({k: (v if not isinstance(v, dict) or "median" not in v else {q: round(v[q], 2) for q in ("median", "min", "max", "spread")})
                              for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()

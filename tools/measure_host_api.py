#!/usr/bin/env python
"""PCIe-inclusive rate of the host-buffer entry point davo_forward: numpy arrays in
pageable host memory -> poses on the host, B=32, 128x416.  Not the bench metric (bench.py keeps the
inputs resident in HBM); reported for information."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                   # noqa: E402
from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION   # noqa: E402



def h2d_bytes_per_window(H, W, pairs):
    """what davo_submit copies per window of the flagship (api.hip: stage_inputs): the strip, the flow planes the path reads, the
    source frames' label maps (batches of four and more; smaller both-pairs batches copy all three) - or, with one pair, the
    (tgt, source) two thirds of every strip row, one flow plane and one label map"""
    hw = H * W
    return hw * 6 + hw * 8 + hw * 4 if pairs != "both" else hw * 9 + hw * 16 + hw * 8


def pairs_measurement(arms, rounds, n=30, H=128, W=416):
    """`--pairs both src1 [--rounds R]`: windows/s of the streamed path (davo_submit from page-locked host memory, the slots
    PoseStream picks: three at B = 32, four at B = 1) for each pair selection, the arms alternating inside every round of one
    process, with the H2D bytes per window beside them.  f16x3 and float32."""
    from davo_amd import pinned_empty
    cfg = parse_version(FLAGSHIP_VERSION)
    weights = synth.make_weights(cfg)
    img, flow, seg = synth.make_inputs(8, H, W)
    for B, slots in ((32, 3), (1, 4)):
        reps = -(-B // 8)
        host = tuple(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B] for a in (img, flow, seg))
        e = Engine(cfg, H, W, B)
        e.load_weights(weights)
        e.set_inflight(slots)
        pinned = tuple(pinned_empty(a.shape, a.dtype) for a in host)
        for d, a in zip(pinned, host):
            d[...] = a
        nb = n if B > 1 else 20 * n
        outs = [np.empty((B, 2, 6), np.float32) for _ in range(nb)]
        for prec in ("f16x3", "f32"):
            e.set_precision(prec)
            rates = {arm: [] for arm in arms}
            for r in range(rounds + 1):                      # round 0 warms up
                for arm in arms:
                    e.set_pairs(arm)
                    t0 = time.perf_counter()
                    for o in outs:
                        e.submit(*pinned, o, hold=8)
                    e.synchronize()
                    if r:
                        rates[arm].append(B * nb / (time.perf_counter() - t0))
            for arm in arms:
                mb = h2d_bytes_per_window(H, W, arm) + (0 if (arm != "both" or B >= 4) else H * W * 4)
                print("davo_submit pinned %-5s B=%-2d %d slots pairs=%-4s: %9.1f windows/s best, rounds %s; %d B H2D per window -> %.1f GB/s"
                      % (prec, B, slots, arm, max(rates[arm]), " ".join("%.0f" % x for x in rates[arm]), mb, mb * max(rates[arm]) / 1e9), flush=True)
        e.close()


def batch1_measurement(calls=3000, H=128, W=416):
    """`--batch1`: host cost of the two host entry points at the reference's operating point, one window per call from
    page-locked memory - us per davo_forward call (one slot) and us per davo_submit on four slots (delivery included), the best
    of three passes of `calls` calls each, f16x3 and float32."""
    from davo_amd import pinned_empty
    cfg = parse_version(FLAGSHIP_VERSION)
    host = synth.make_inputs(1, H, W)
    pinned = tuple(pinned_empty(a.shape, a.dtype) for a in host)
    for d, a in zip(pinned, host):
        d[...] = a
    e = Engine(cfg, H, W, 1)
    e.load_weights(synth.make_weights(cfg))
    outs = [np.empty((1, 2, 6), np.float32) for _ in range(calls)]
    for prec in ("f16x3", "f32"):
        e.set_precision(prec)
        e.set_inflight(1)
        for _ in range(200):
            e.forward(*pinned)
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(calls):
                e.forward(*pinned)
            best = min(best, (time.perf_counter() - t0) / calls * 1e6)
        print("host_b1 forward_%s_us %.2f" % (prec, best), flush=True)
        e.set_inflight(4)
        best = float("inf")
        for rep in range(4):                                 # pass 0 warms up
            t0 = time.perf_counter()
            for o in outs:
                e.submit(*pinned, o, hold=8)
            e.synchronize()
            if rep:
                best = min(best, (time.perf_counter() - t0) / calls * 1e6)
        print("host_b1 submit_%s_us %.2f" % (prec, best), flush=True)
    e.close()


if "--batch1" in sys.argv:
    batch1_measurement()
    sys.exit(0)

if "--pairs" in sys.argv:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", nargs="+", choices=sorted(Engine.PAIRS), required=True)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    pairs_measurement(args.pairs, args.rounds)
    sys.exit(0)

B = 32
cfg = parse_version(FLAGSHIP_VERSION)
img, flow, seg = synth.make_inputs(8, 128, 416)
img, flow, seg = np.tile(img, (4, 1, 1, 1)), np.tile(flow, (4, 1, 1, 1, 1)), np.tile(seg, (4, 1, 1, 1, 1))
from davo_amd import pinned_empty                                     # noqa: E402

e = Engine(cfg, 128, 416, B)
e.load_weights(synth.make_weights(cfg))
pinned = tuple(pinned_empty(a.shape, a.dtype) for a in (img, flow, seg))
for d, a in zip(pinned, (img, flow, seg)):
    d[...] = a
mb = (img.nbytes + flow.nbytes // 2 + seg.nbytes) / 1e6              # flow planes 2,3 are never read and never copied
n = 30
for label, bufs in (("pageable", (img, flow, seg)), ("pinned", pinned)):
    for chunk in (0, 8):
        e.set_option("host_chunk", chunk)
        for _ in range(3):
            ref = e.forward(*bufs)
        t0 = time.perf_counter()
        for _ in range(n):
            e.forward(*bufs)
        dt = time.perf_counter() - t0
        print("davo_forward host buffers %-8s host_chunk=%d: %8.1f triplets/s, %.3f ms per batch of %d, %.1f MB H2D per batch -> %.1f GB/s"
              % (label, chunk, B * n / dt, dt / n * 1e3, B, mb, mb * n / dt / 1e3), flush=True)

# round 5: the streaming entry point on the same batch (davo_submit, four slots; pinned arrays held for the whole run: hold = 8)
for prec in ("f16x3", "f32"):
    e.set_precision(prec)
    outs = [np.empty((B, 2, 6), np.float32) for _ in range(n)]
    for slots in (1, 2, 3, 4):
        e.set_inflight(slots)
        for rep in range(2):
            t0 = time.perf_counter()
            for o in outs:
                e.submit(*pinned, o, hold=8)
            e.synchronize()
            dt = time.perf_counter() - t0
        print("davo_submit   host buffers pinned   %-5s %d slot(s)    : %8.1f triplets/s, %.3f ms per batch of %d (PCIe-inclusive)"
              % (prec, slots, B * n / dt, dt / n * 1e3, B), flush=True)
    e.set_inflight(1)
    e.set_option("host_chunk", 8)
    e.forward(*pinned)
    t0 = time.perf_counter()
    for _ in range(n):
        e.forward(*pinned)
    dt = time.perf_counter() - t0
    print("davo_forward  host buffers pinned   %-5s host_chunk=8 : %8.1f triplets/s, %.3f ms per batch of %d (PCIe-inclusive)"
          % (prec, B * n / dt, dt / n * 1e3, B), flush=True)

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
    """what davo_submit copies per window of the flagship (entry.hip: stage_inputs): the strip, the flow planes the path reads, the
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


def labels_measurement(arms, rounds, n=30, H=128, W=416):
    """`--labels f32 u8 [--rounds R]`: the label formats (davo_set_label_format) against each other, one engine per format in ONE
    process, the arms alternating inside every round (round 0 warms up), f16x3 and float32:
      resident  ms per davo_forward_device step at B = 32 with the inputs in HBM (the bench's path): per arm the median, and the
                spread (max - min) of its rounds - the margin of the "byte labels are not slower" bound;
      streamed  windows/s of davo_submit from page-locked memory at B = 32 and at batch 1, with 1..4 slots, best of the rounds,
                beside the H2D bytes per window;
    and once per format the device memory a context holds after streaming on four slots (staging sets + the guard's snapshots)."""
    import ctypes
    from davo_amd import pinned_empty
    from davo_amd import _lib
    from davo_amd.labels import LABEL_DTYPES
    _lib.lib()                                               # loads the HIP runtime free_bytes asks

    def free_bytes():
        hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
        return free.value

    cfg = parse_version(FLAGSHIP_VERSION)
    weights = synth.make_weights(cfg)
    hw = H * W
    for B in (32, 1):
        engines, host, pinned, dev = {}, {}, {}, {}
        for arm in arms:
            img, flow, seg = synth.make_inputs(min(8, B), H, W, labels=arm)
            reps = -(-B // 8)
            host[arm] = tuple(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B] for a in (img, flow, seg))
            before = free_bytes()
            e = engines[arm] = Engine(cfg, H, W, B, labels=arm)
            e.load_weights(weights)
            pinned[arm] = tuple(pinned_empty(a.shape, a.dtype) for a in host[arm])
            for d, a in zip(pinned[arm], host[arm]):
                d[...] = a
            e.set_inflight(4)
            outs = [np.empty((B, 2, 6), np.float32) for _ in range(5)]
            for o in outs:
                e.submit(*pinned[arm], o, hold=8)
            e.synchronize()
            lab = LABEL_DTYPES[arm].itemsize
            print("labels=%-3s B=%-2d: %d B of device memory held by the context after streaming on 4 slots; a window's label maps "
                  "%d B, a staging set's %d B, the eight snapshots' %d B" % (arm, B, before - free_bytes(), 3 * hw * lab, 3 * hw * lab * B, 8 * 3 * hw * lab * B), flush=True)
            dev[arm] = tuple(e.alloc(a.nbytes).upload(a) for a in host[arm]) + (e.alloc(B * 48),)
        nb = n if B > 1 else 20 * n
        outs = [np.empty((B, 2, 6), np.float32) for _ in range(nb)]
        for prec in ("f16x3", "f32"):
            for e in engines.values():
                e.set_precision(prec)
            if B == 32:
                step = {arm: [] for arm in arms}
                for e in engines.values():
                    e.set_inflight(1)
                for r in range(rounds + 1):
                    for arm in arms:
                        e = engines[arm]
                        for _ in range(5):
                            e.forward_device(B, *dev[arm])
                        e.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(n):
                            e.forward_device(B, *dev[arm])
                        e.synchronize()
                        if r:
                            step[arm].append((time.perf_counter() - t0) / n * 1e3)
                for arm in arms:
                    v = sorted(step[arm])
                    print("resident davo_forward_device %-5s B=%d labels=%-3s: median %.4f ms per step, spread %.4f (rounds %s)"
                          % (prec, B, arm, v[len(v) // 2], v[-1] - v[0], " ".join("%.4f" % x for x in step[arm])), flush=True)
            for slots in (1, 2, 3, 4):
                rates = {arm: [] for arm in arms}
                for e in engines.values():
                    e.set_inflight(slots)
                for r in range(rounds + 1):
                    for arm in arms:
                        e = engines[arm]
                        t0 = time.perf_counter()
                        for o in outs:
                            e.submit(*pinned[arm], o, hold=8)
                        e.synchronize()
                        if r:
                            rates[arm].append(B * nb / (time.perf_counter() - t0))
                for arm in arms:
                    lab = LABEL_DTYPES[arm].itemsize
                    mb = hw * 9 + hw * 16 + hw * lab * (2 if B >= 4 else 3)
                    print("davo_submit pinned %-5s B=%-2d %d slot(s) labels=%-3s: %9.1f windows/s best, rounds %s; %d B H2D per window -> %.1f GB/s"
                          % (prec, B, slots, arm, max(rates[arm]), " ".join("%.0f" % x for x in rates[arm]), mb, mb * max(rates[arm]) / 1e9), flush=True)
        for e in engines.values():
            e.close()


def layout_measurement(arms, rounds, n=30, H=128, W=416):
    """`--layout windows frames [--rounds R]` (default: windows only): the frame layout (include/davo_hip.h "Frame sequences")
    against the window layout, ONE engine per label format (window and frame calls mix freely on a context), the arms alternating
    inside every round (round 0 warms up), f16x3 and float32, float and byte labels:
      resident  ms per davo_forward_device / davo_forward_device_frames step at B = 32 with the inputs in HBM: per arm the median
                and the spread (max - min) of its rounds.  The difference of the medians is what the gather costs;
      streamed  windows/s of davo_submit / davo_submit_frames from page-locked memory at B = 32 and at batch 1, with 1..4 slots,
                best of the rounds, beside the H2D bytes per window (davo_frames_plan's for the frame arm)."""
    from davo_amd import frames_plan, pinned_empty, windows_from_frames
    cfg = parse_version(FLAGSHIP_VERSION)
    weights = synth.make_weights(cfg)
    hw = H * W
    for labels in ("f32", "u8"):
        lab = 4 if labels == "f32" else 1
        for B in (32, 1):
            fr = synth.make_frames(B + 2, H, W, labels=labels)
            host = {"frames": fr, "windows": windows_from_frames(*fr)}
            e = Engine(cfg, H, W, B, labels=labels)
            e.load_weights(weights)
            pinned = {arm: tuple(pinned_empty(a.shape, a.dtype) for a in host[arm]) for arm in arms}
            dev = {}
            for arm in arms:
                for d, a in zip(pinned[arm], host[arm]):
                    d[...] = a
                dev[arm] = tuple(e.alloc(a.nbytes).upload(a) for a in host[arm]) + (e.alloc(B * 48),)
            issue = {"windows": e.submit, "frames": e.submit_frames}
            step_fn = {"windows": e.forward_device, "frames": e.forward_device_frames}
            link = {"windows": hw * 9 + hw * 16 + hw * lab * (2 if B >= 4 else 3),
                    "frames": frames_plan(H, W, B, "both", cfg.att_source, labels)["link_bytes"] // B}
            nb = n if B > 1 else 20 * n
            outs = [np.empty((B, 2, 6), np.float32) for _ in range(nb)]
            for prec in ("f16x3", "f32"):
                e.set_precision(prec)
                if B == 32:
                    e.set_inflight(1)
                    step = {arm: [] for arm in arms}
                    for r in range(rounds + 1):
                        for arm in arms:
                            for _ in range(5):
                                step_fn[arm](B, *dev[arm])
                            e.synchronize()
                            t0 = time.perf_counter()
                            for _ in range(n):
                                step_fn[arm](B, *dev[arm])
                            e.synchronize()
                            if r:
                                step[arm].append((time.perf_counter() - t0) / n * 1e3)
                    for arm in arms:
                        v = sorted(step[arm])
                        print("resident %-7s %-5s B=%d labels=%-3s: median %.4f ms per step, spread %.4f (rounds %s)"
                              % (arm, prec, B, labels, v[len(v) // 2], v[-1] - v[0], " ".join("%.4f" % x for x in step[arm])), flush=True)
                for slots in (1, 2, 3, 4):
                    e.set_inflight(slots)
                    rates = {arm: [] for arm in arms}
                    for r in range(rounds + 1):
                        for arm in arms:
                            t0 = time.perf_counter()
                            for o in outs:
                                issue[arm](*pinned[arm], o, hold=8)
                            e.synchronize()
                            if r:
                                rates[arm].append(B * nb / (time.perf_counter() - t0))
                    for arm in arms:
                        print("streamed %-7s %-5s B=%-2d %d slot(s) labels=%-3s: %9.1f windows/s best, rounds %s; %d B H2D per window -> %.1f GB/s"
                              % (arm, prec, B, slots, labels, max(rates[arm]), " ".join("%.0f" % x for x in rates[arm]), link[arm],
                                 link[arm] * max(rates[arm]) / 1e9), flush=True)
            e.close()


def flow_measurement(arms, rounds, n=30, H=128, W=416):
    """`--flow f32 f16 [--rounds R]`: the flow formats (davo_set_flow_format) against each other, byte labels, one engine per
    format in ONE process, the arms alternating inside every round (round 0 warms up), f16x3 and float32:
      resident  ms per davo_forward_device step at B = 32 with the inputs in HBM (the bench's path): per arm the median, and the
                spread (max - min) of its rounds - the margin of the "binary16 flow is not slower" bound; then, profiled, the
                mean launch time of the squeeze and of mask_pack (davo_profile_entry);
      streamed  windows/s of davo_submit (window layout) and davo_submit_frames (frame layout) from page-locked memory at B = 32
                and at batch 1, with 1, 2 and 4 slots, best of the rounds, beside the H2D bytes per window.
    The float32 arm on flow_from_f16 of the binary16 arm's halves computes the same bits (tests/test_f16_flow_gpu.py)."""
    from davo_amd import flow_from_f16, frames_plan, pinned_empty, windows_from_frames
    cfg = parse_version(FLAGSHIP_VERSION)
    weights = synth.make_weights(cfg)
    hw = H * W
    for B in (32, 1):
        engines, pinned, dev, link = {}, {}, {}, {}
        fr16 = synth.make_frames(B + 2, H, W, labels="u8", flow="f16")
        for arm in arms:
            fr = fr16 if arm == "f16" else (fr16[0], flow_from_f16(fr16[1]), fr16[2])
            host = {"windows": windows_from_frames(*fr), "frames": fr}
            e = engines[arm] = Engine(cfg, H, W, B, labels="u8", flow=arm)
            e.load_weights(weights)
            pinned[arm] = {k: tuple(pinned_empty(a.shape, a.dtype) for a in v) for k, v in host.items()}
            for k in host:
                for d, a in zip(pinned[arm][k], host[k]):
                    d[...] = a
            dev[arm] = tuple(e.alloc(a.nbytes).upload(a) for a in host["windows"]) + (e.alloc(B * 48),)
            fb = 2 if arm == "f16" else 4
            link[arm] = {"windows": hw * 9 + hw * 4 * fb + hw * (2 if B >= 4 else 3),
                         "frames": frames_plan(H, W, B, "both", cfg.att_source, "u8", arm)["link_bytes"] // B}
        nb = n if B > 1 else 20 * n
        outs = [np.empty((B, 2, 6), np.float32) for _ in range(nb)]
        for prec in ("f16x3", "f32"):
            for e in engines.values():
                e.set_precision(prec)
            if B == 32:
                step = {arm: [] for arm in arms}
                for e in engines.values():
                    e.set_inflight(1)
                for r in range(rounds + 1):
                    for arm in arms:
                        e = engines[arm]
                        for _ in range(5):
                            e.forward_device(B, *dev[arm])
                        e.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(n):
                            e.forward_device(B, *dev[arm])
                        e.synchronize()
                        if r:
                            step[arm].append((time.perf_counter() - t0) / n * 1e3)
                for arm in arms:
                    v = sorted(step[arm])
                    print("resident davo_forward_device %-5s B=%d flow=%-3s: median %.4f ms per step, spread %.4f (rounds %s)"
                          % (prec, B, arm, v[len(v) // 2], v[-1] - v[0], " ".join("%.4f" % x for x in step[arm])), flush=True)
                for arm in arms:                             # the launches that read raw flow, bracketed by events
                    e = engines[arm]
                    e.profile(1)
                    e.profile_reset()
                    for _ in range(n):
                        e.forward_device(B, *dev[arm])
                    e.synchronize()
                    ent = e.profile_entries()
                    e.profile(0)
                    print("profiled %-5s B=%d flow=%-3s: %s" % (prec, B, arm, "  ".join(
                        "%s %.1f us x %d" % (k, 1e3 * ent[k][1] / max(ent[k][0], 1), ent[k][0]) for k in ("se_squeeze_partial", "mask_pack", "cnv1") if k in ent)), flush=True)
            for layout, issue in (("windows", "submit"), ("frames", "submit_frames")):
                for slots in (1, 2, 4):
                    rates = {arm: [] for arm in arms}
                    for e in engines.values():
                        e.set_inflight(slots)
                    for r in range(rounds + 1):
                        for arm in arms:
                            e = engines[arm]
                            t0 = time.perf_counter()
                            for o in outs:
                                getattr(e, issue)(*pinned[arm][layout], o, hold=8)
                            e.synchronize()
                            if r:
                                rates[arm].append(B * nb / (time.perf_counter() - t0))
                    for arm in arms:
                        mb = link[arm][layout]
                        print("streamed %-7s %-5s B=%-2d %d slot(s) flow=%-3s: %9.1f windows/s best, rounds %s; %d B H2D per window -> %.1f GB/s"
                              % (layout, prec, B, slots, arm, max(rates[arm]), " ".join("%.0f" % x for x in rates[arm]), mb, mb * max(rates[arm]) / 1e9), flush=True)
        for e in engines.values():
            e.close()


if "--flow" in sys.argv:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--flow", nargs="+", choices=("f32", "f16"), required=True)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    flow_measurement(args.flow, args.rounds)
    sys.exit(0)

if "--layout" in sys.argv:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", nargs="+", choices=("windows", "frames"), default=["windows"])
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    layout_measurement(args.layout, args.rounds)
    sys.exit(0)

if "--batch1" in sys.argv:
    batch1_measurement()
    sys.exit(0)

if "--labels" in sys.argv:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", nargs="+", choices=("f32", "u8"), required=True)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    labels_measurement(args.labels, args.rounds)
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

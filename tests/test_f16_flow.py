"""Binary16 optical flow without a GPU (include/davo_hip.h: davo_set_flow_format): the one host-side rounding rule and its
widening twin, the C surface, the frame plan's byte counts, the synthetic inputs, the loaders, the driver's option - and what
the opt-in costs in the poses, measured on the float64 oracle.

The rounding rule is checked against a restatement in exact rational arithmetic: the nearest binary16 value, ties to the even
significand, finite values beyond +-65504 to +-65504."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import davo_amd
from davo_amd import _lib, frames_plan, loader as L, synth
from davo_amd.flow import FLOW_DTYPES, flow_from_f16, flow_to_f16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_halves():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def _bits16(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def _one(x):
    """the bit pattern of flow_to_f16 of one value"""
    return int(_bits16(flow_to_f16(np.float32([x])))[0])


_TABLE = []


def _half_table():
    """every finite half but -0, sorted: (exact value, bit pattern)"""
    if not _TABLE:
        halves = _all_halves()
        keep = np.isfinite(halves) & (_bits16(halves) != 0x8000)
        _TABLE.extend(sorted((Fraction(v), b) for v, b in zip(halves[keep].astype(np.float64).tolist(), _bits16(halves)[keep].tolist())))
    return _TABLE


def _nearest_even_half(x):
    """the rule, one finite value at a time in exact arithmetic over the sorted finite halves: -> the half's bit pattern"""
    table = _half_table()
    v = Fraction(float(np.float32(x)))
    if v >= table[-1][0]:
        return table[-1][1]
    if v <= table[0][0]:
        return table[0][1]
    lo, hi = 0, len(table) - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if table[mid][0] <= v:
            lo = mid
        else:
            hi = mid
    (a, abits), (b, bbits) = table[lo], table[hi]
    if v - a != b - v:
        bits = abits if v - a < b - v else bbits
    else:
        bits = abits if abits % 2 == 0 else bbits        # the tie goes to the even significand
    if bits == 0 and np.signbit(np.float32(x)):
        bits = 0x8000                                        # a result that rounds to zero keeps the sign
    return bits


def test_the_rule_rounds_to_nearest_even_and_saturates():
    one_ulp = 2.0 ** -10                                     # spacing of the halves in [1, 2)
    ties = [1 + one_ulp / 2, 1 + 3 * one_ulp / 2, -(1 + one_ulp / 2), -(1 + 3 * one_ulp / 2), 2048 + 1.0, 2048 + 3.0, 65504 - 16.0,
            2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -24 + 2.0 ** -25, 1023.5 * 2.0 ** -24]      # the last ones tie between subnormals
    for v, want in ((1 + one_ulp / 2, 0x3C00), (1 + 3 * one_ulp / 2, 0x3C02), (2049.0, 0x6800), (2051.0, 0x6802),
                    (2.0 ** -25, 0x0000), (3 * 2.0 ** -25, 0x0002), (-(2.0 ** -25), 0x8000)):
        assert _one(v) == want, v
    rng = np.random.default_rng(20261020)
    values = np.concatenate([np.asarray(ties, np.float32), rng.normal(0.3, 15.4, 3000).astype(np.float32),
                             (rng.uniform(-1, 1, 500) * 2.0 ** -14).astype(np.float32),       # around the subnormal range
                             (rng.uniform(-1, 1, 300) * 2.0 ** -23).astype(np.float32),
                             rng.uniform(-70000, 70000, 500).astype(np.float32)])
    got = _bits16(flow_to_f16(values))
    want = np.array([_nearest_even_half(v) for v in values], np.uint16)
    assert np.array_equal(got, want), values[got != want][:5]
    # saturation: at +-65504 and beyond; binary16 itself would round 65520 and more to infinity
    for v in (65504.0, 65519.99, 65520.0, 70000.0, 1e9, 3.4e38):
        assert _one(v) == 0x7BFF and _one(-v) == 0xFBFF, v
    assert np.isfinite(flow_to_f16(values)).all()            # a finite flow stays finite
    # NaN stays NaN, an infinity that infinity, zeros keep their sign, small results are subnormals
    sp = flow_to_f16(np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0 ** -24, -1023 * 2.0 ** -24, 1e-30, -1e-30]))
    assert np.isnan(sp[0]) and list(_bits16(sp[1:])) == [0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x83FF, 0x0000, 0x8000]
    shaped = flow_to_f16(np.zeros((2, 4, 4, 8, 2), np.float32))
    assert shaped.shape == (2, 4, 4, 8, 2) and shaped.dtype == np.float16
    assert davo_amd.flow_to_f16 is flow_to_f16 and davo_amd.flow_from_f16 is flow_from_f16      # one definition


def test_widening_is_exact_for_every_half():
    h = _all_halves()
    w = flow_from_f16(h)
    assert w.dtype == np.float32 and w.shape == h.shape
    nan = np.isnan(h)
    assert nan.sum() == 2 * 1023 and np.isnan(w[nan]).all()
    assert np.array_equal(_bits16(flow_to_f16(w))[~nan], _bits16(h)[~nan])       # round(widen(x)) == x, every bit pattern that is not NaN
    # ... and the widened value IS the half's value: sign, exponent and significand decoded by hand
    bits = _bits16(h).astype(np.int64)
    sign, ex, man = np.where(bits >> 15, -1.0, 1.0), (bits >> 10) & 31, bits & 1023
    value = np.where(ex == 0, man * 2.0 ** -24, (1024 + man) * 2.0 ** (ex.astype(np.float64) - 25))
    fin = ex < 31
    assert np.array_equal(w[fin].astype(np.float64), (sign * value)[fin]) and np.array_equal(np.signbit(w[fin]), bits[fin] >> 15 == 1)
    assert np.array_equal(w[(ex == 31) & (man == 0)], np.float32([np.inf, -np.inf]))
    with pytest.raises(ValueError, match="float16"):
        flow_from_f16(np.zeros(4, np.float32))


def test_surface():
    header = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    assert re.search(r"int davo_set_flow_format\(davo_ctx\* ctx, int fmt\);", header)
    assert re.search(r"int davo_get_flow_format\(const davo_ctx\* ctx\);", header)
    assert re.search(r"DAVO_FLOW_F32 = 0\b", header) and re.search(r"DAVO_FLOW_F16 = 1\b", header)
    assert re.search(r"int davo_frames_plan_fmt\(int H, int W, int N, int pairs, int att_source, int label_fmt, int flow_fmt, int\* ranges, long long\* link_bytes\);", header)
    for figure in ("1,011,712", "638,976", "425,984", "479,232", "106,496", "159,744", "53,248"):      # the byte counts a caller plans with
        assert figure in header, figure
    assert (_lib.FLOW_F32, _lib.FLOW_F16) == (0, 1)
    for name in ("davo_set_flow_format", "davo_get_flow_format", "davo_frames_plan_fmt"):
        assert name in _lib.EXPORTS
    lib = _lib.lib()
    assert lib.davo_set_flow_format.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.davo_get_flow_format.argtypes == [ctypes.c_void_p]
    raw = ctypes.CDLL(_lib.LIB_PATH)                         # the library's own export table, not the binding's list
    assert raw.davo_set_flow_format and raw.davo_get_flow_format and raw.davo_frames_plan_fmt
    assert lib.davo_set_flow_format(None, 1) == -1 and lib.davo_get_flow_format(None) == -1      # no context: DAVO_ERR_INVALID
    assert callable(davo_amd.Engine.set_flow_format) and callable(davo_amd.DAVO.use_f16_flow)


def _plan_table(N, pairs, tgt_attended):
    """the header's table ("Frame sequences"), no depth: frames, flow planes and label maps [lo, hi) a batch of N windows reads"""
    if pairs == "both":
        return (0, N + 2), (0, 2), (0, N + 2)
    if pairs == "src0":
        return (0, N + 1), (0, 1), (0, N + 1) if tgt_attended else (0, N)
    return (1, N + 2), (1, 2), (1, N + 2) if tgt_attended else (2, N + 2)


@pytest.mark.parametrize("labels", ["f32", "u8"])
@pytest.mark.parametrize("pairs", ["both", "src0", "src1"])
def test_frames_plan_fmt_is_the_headers_table(pairs, labels):
    H, W = 128, 416
    for att, tgt in (("se_flow", False), ("static_all", True)):
        for N in (1, 7, 64):
            frames, flow, seg = _plan_table(N, pairs, tgt)
            for fmt, per in (("f32", 4), ("f16", 2)):
                p = frames_plan(H, W, N, pairs, att, labels, fmt)
                assert (p["frames"], p["flow"], p["seg"], p["depth"]) == (frames, flow, seg, (0, 0)), (att, N, fmt)
                want = (frames[1] - frames[0]) * H * W * 3 + N * (flow[1] - flow[0]) * H * W * 2 * per + \
                       (seg[1] - seg[0]) * H * W * (1 if labels == "u8" else 4)
                assert p["link_bytes"] == want, (att, N, fmt)
            # davo_frames_plan is flow_fmt = 0
            lib, r0, r1 = _lib.lib(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
            b0, b1 = ctypes.c_longlong(0), ctypes.c_longlong(0)
            code = {"src0": 1, "src1": 2, "both": 3}[pairs]
            a = davo_amd.version.ATT_SOURCE[att]
            assert lib.davo_frames_plan(H, W, N, code, a, labels == "u8", r0, ctypes.byref(b0)) == 0
            assert lib.davo_frames_plan_fmt(H, W, N, code, a, labels == "u8", 0, r1, ctypes.byref(b1)) == 0
            assert list(r0) == list(r1) and b0.value == b1.value == frames_plan(H, W, N, pairs, att, labels)["link_bytes"]
            assert lib.davo_frames_plan_fmt(H, W, N, code, a, labels == "u8", 2, r1, ctypes.byref(b1)) == -1
            assert lib.davo_frames_plan_fmt(H, W, N, code, a, labels == "u8", -1, None, None) == -1


def test_the_byte_counts_a_caller_plans_with():
    """include/davo_hip.h, per window at 128x416, both pairs, byte labels (a long batch: the two extra frames are not counted)"""
    H, W = 128, 416
    HW = H * W
    assert (9 * HW, 2 * HW * 2 * 2, 2 * HW) == (479232, 425984, 106496) and 479232 + 425984 + 106496 == 1011712      # window form
    assert 9 * HW + 2 * HW * 2 * 4 + 2 * HW == 1437696                                                                # ... float32 flow
    per_window = lambda **kw: frames_plan(H, W, 1001, "both", "se_flow", "u8", **kw)["link_bytes"] - frames_plan(H, W, 1000, "both", "se_flow", "u8", **kw)["link_bytes"]      # noqa: E731
    assert per_window(flow="f16") == 159744 + 425984 + 53248 == 638976
    assert per_window() == per_window(flow="f32") == 1064960
    assert round(100 * (1 - 638976 / 1064960)) == 40
    with pytest.raises(ValueError, match="flow"):
        frames_plan(H, W, 4, flow="bf16")


def test_synthetic_inputs():
    img, flow, seg = synth.make_inputs(2, 16, 24, first_window=5)
    img16, flow16, seg16 = synth.make_inputs(2, 16, 24, first_window=5, flow="f16")
    assert flow16.dtype == np.float16 and flow16.shape == flow.shape
    assert np.array_equal(_bits16(flow16), _bits16(flow_to_f16(flow))) and np.array_equal(img16, img) and np.array_equal(seg16, seg)
    assert not np.array_equal(flow_from_f16(flow16), flow) and np.abs(flow_from_f16(flow16) - flow).max() < 0.05
    both = synth.make_inputs(2, 16, 24, first_window=5, flow="f16", labels="u8")
    assert both[1].dtype == np.float16 and both[2].dtype == np.uint8
    fr, fr16 = synth.make_frames(5, 16, 24), synth.make_frames(5, 16, 24, flow="f16")
    assert fr16[1].dtype == np.float16 and np.array_equal(_bits16(fr16[1]), _bits16(flow_to_f16(fr[1])))
    assert np.array_equal(fr16[0], fr[0]) and np.array_equal(fr16[2], fr[2])
    win = davo_amd.windows_from_frames(*fr16)                # the conversions keep the dtype
    assert win[1].dtype == np.float16 and np.array_equal(_bits16(win[1][:, :2]), _bits16(fr16[1])) and not win[1][:, 2:].any()
    assert davo_amd.frames_from_windows(*win)[1].dtype == np.float16
    for fn in (lambda: synth.make_inputs(1, 16, 24, flow="bf16"), lambda: synth.make_frames(4, 16, 24, flow="f64")):
        with pytest.raises(ValueError, match="flow"):
            fn()


H, W, FRAMES, B = 16, 24, 9, 3                               # 7 windows: two whole batches and a short one


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """a float32 dump, its binary16 twin and the float32 dump of the twin's widened values; two sequences each"""
    out = {}
    for fmt in ("f32", "f16", "widened"):
        out[fmt] = str(tmp_path_factory.mktemp("dump_" + fmt))
        for seq, seed in ((3, 11), (4, 12)):
            L.write_synthetic_dump(out[fmt], seq, FRAMES, H, W, seed=seed, flow=fmt)
    return out


def test_the_half_dump_is_the_float_dumps_twin(dumps):
    for w in (1, FRAMES - 2):
        a, b, c = (np.load(L.window_paths(dumps[k], 3, w)[1]) for k in ("f32", "f16", "widened"))
        assert a.dtype == np.float32 and b.dtype == np.float16 and c.dtype == np.float32 and a.shape == b.shape == c.shape == (4, H, W, 2)
        assert np.array_equal(_bits16(b), _bits16(flow_to_f16(a))) and np.array_equal(c, flow_from_f16(b))
        for k in (0, 2):                                     # strips and label maps are the same files
            assert open(L.window_paths(dumps["f32"], 3, w)[k], "rb").read() == open(L.window_paths(dumps["f16"], 3, w)[k], "rb").read()
    with pytest.raises(ValueError, match="flow"):
        L.write_synthetic_dump(dumps["f32"], 9, 3, H, W, flow="bf16")


def _collect(loader):
    out = []
    for s, e, parts in loader:
        out.append((s, e, tuple(np.array(p) for p in parts)))
    return out


def test_threaded_loader(dumps):
    want = _collect(L.kitti_loader(dumps["f32"], 3, H, W, 0, FRAMES - 2, B, workers=2))
    assert [(s, e) for s, e, _ in want] == [(0, 3), (3, 6), (6, 7)] and want[0][2][1].dtype == np.float32
    for dump in ("f16", "f32"):                              # read as it is; converted by the worker
        got = _collect(L.kitti_loader(dumps[dump], 3, H, W, 0, FRAMES - 2, B, workers=2, flow="f16"))
        assert len(got) == len(want)
        for (s, e, g), (s0, e0, w) in zip(got, want):
            assert (s, e) == (s0, e0) and g[1].dtype == np.float16 and g[1].shape == w[1].shape
            assert np.array_equal(_bits16(g[1]), _bits16(flow_to_f16(w[1]))) and np.array_equal(g[0], w[0]) and np.array_equal(g[2], w[2])
    one = L.load_window(dumps["f16"], 3, 1, H, W, flow="f16")[1]
    assert one.dtype == np.float16 and np.array_equal(_bits16(one), _bits16(flow_to_f16(L.load_window(dumps["f32"], 3, 1, H, W)[1])))
    both = L.load_window(dumps["f32"], 3, 1, H, W, labels="u8", flow="f16")
    assert both[1].dtype == np.float16 and both[2].dtype == np.uint8


def _process_batches(dump, flow, segments=None, flow_planes=L.FLOW_PLANES_USED, labels="f32"):
    if segments is None:
        ld = L.ProcessWindowLoader(dump, 3, H, W, 0, FRAMES - 2, B, procs=2, flow_planes=flow_planes, flow=flow, labels=labels)
    else:
        ld = L.ProcessWindowLoader(dump, None, H, W, None, None, B, procs=2, flow_planes=flow_planes, flow=flow, labels=labels, segments=segments)
    try:
        return [_collect(ld)] if segments is None else [_collect(ld.segment(k)) for k in range(len(segments))]
    finally:
        ld.close()


def test_process_loader(dumps):
    want = _process_batches(dumps["f32"], "f32")
    for dump in ("f16", "f32"):
        got = _process_batches(dumps[dump], "f16")
        assert [(s, e) for s, e, _ in got[0]] == [(0, 3), (3, 6), (6, 7)]
        for (s, e, g), (_, _, w) in zip(got[0], want[0]):
            assert g[1].dtype == np.float16 and np.array_equal(_bits16(g[1]), _bits16(flow_to_f16(w[1]))), (dump, s)
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[2], w[2])
            assert not g[1][:, 2:].any() and g[1][:, :2].any()      # flow planes 0, 1 alone: the others are never read
    # every plane, two segments from one pool, with byte labels
    segments = [(3, 0, FRAMES - 2), (4, 2, 6)]
    want2 = _process_batches(dumps["f32"], "f32", segments, flow_planes=None)
    for dump in ("f16", "f32"):
        got2 = _process_batches(dumps[dump], "f16", segments, flow_planes=None, labels="u8")
        for k in range(2):
            assert [(s, e) for s, e, _ in got2[k]] == [(s, e) for s, e, _ in want2[k]]
            for (_, _, g), (_, _, w) in zip(got2[k], want2[k]):
                assert np.array_equal(_bits16(g[1]), _bits16(flow_to_f16(w[1]))) and g[1][:, 3].any() and g[2].dtype == np.uint8


def test_process_loader_flow_segments_hold_half_the_bytes(dumps):
    sizes = {}
    for fmt in ("f32", "f16"):
        ld = L.ProcessWindowLoader(dumps["f32"], 3, H, W, 0, FRAMES - 2, B, procs=1, flow=fmt)
        ld.start()
        try:
            sizes[fmt] = [v[1].nbytes for v in ld._views]
            assert all(v[1].dtype == FLOW_DTYPES[fmt] for v in ld._views)
            assert all(trio[1].size >= v[1].nbytes for trio, v in zip(ld._segs, ld._views))
            assert all(trio[1].size < 2 * v[1].nbytes for trio, v in zip(ld._segs, ld._views)) or fmt == "f32"
        finally:
            ld.close()
    assert len(sizes["f16"]) == len(sizes["f32"]) > 0
    assert all(2 * a == b == B * 4 * H * W * 2 * 4 for a, b in zip(sizes["f16"], sizes["f32"]))


def test_any_other_flow_dtype_is_an_error_that_names_the_file(dumps, tmp_path):
    bad = str(tmp_path / "bad")
    shutil.copytree(dumps["f32"], bad)
    path = L.window_paths(bad, 3, 2)[1]
    np.save(path, np.load(path).astype(np.float64))
    with pytest.raises(ValueError, match=re.escape(path)):
        L.load_window(bad, 3, 2, H, W, flow="f16")
    with pytest.raises(ValueError, match=re.escape(path)):
        _collect(L.kitti_loader(bad, 3, H, W, 0, FRAMES - 2, B, workers=2, flow="f16"))
    with pytest.raises(ValueError, match=re.escape(path)):
        _process_batches(bad, "f16")
    with pytest.raises(ValueError, match="flow"):
        L.kitti_loader(dumps["f32"], 3, H, W, 0, 1, B, flow="half")
    with pytest.raises(ValueError, match="flow"):
        L.ProcessWindowLoader(dumps["f32"], 3, H, W, 0, 1, B, flow="half")
    with pytest.raises(ValueError, match="flow slot"):       # a float32 slot handed over as a binary16 one
        L.load_window_into(dumps["f32"], 3, 1, H, W, np.empty((H, 3 * W, 3), np.uint8), np.empty((4, H, W, 2), np.float32),
                           np.empty((3, H, W, 1), np.float32), flow_fmt="f16")


def test_a_trajectory_from_halves_is_the_widened_dumps_to_the_byte(dumps, tmp_path):
    """The driver has no CPU path (the library is the only implementation), so the sequence loop of run_kitti_pose runs here on
    the float64 oracle: the window loaders in both formats, the stitch and the file writer.  A float16 dump read as halves and
    widened, a float32 dump rounded by the loader and widened, and the float32 dump of the widened values must write one file."""
    from davo_amd import sequence as S
    from oracle import c_oracle
    cfg = davo_amd.parse_version(davo_amd.FLAGSHIP_VERSION)
    weights = synth.make_weights(cfg)
    files = []
    for dump, fmt in (("widened", "f32"), ("f16", "f16"), ("f32", "f16")):
        def infer(img, flow, seg, fmt=fmt):
            assert flow.dtype == FLOW_DTYPES[fmt]
            return c_oracle.forward(cfg, img, flow_from_f16(flow) if fmt == "f16" else flow, seg, weights)
        load = S.kitti_window_loader(dumps[dump], 3, FRAMES, H, W, workers=2, flow=fmt)
        traj, _ = S.run_sequence(infer, load, FRAMES, B)
        out = str(tmp_path / ("%s_%s.txt" % (dump, fmt)))
        S.write_kitti_poses(out, traj)
        files.append(open(out, "rb").read())
    assert len(files[0]) > 0 and files[1] == files[0] and files[2] == files[0]
    # ... and the float32 dump itself gives another file: the rounding is real
    traj, _ = S.run_sequence(lambda i, f, s: c_oracle.forward(cfg, i, f, s, weights), S.kitti_window_loader(dumps["f32"], 3, FRAMES, H, W, workers=2), FRAMES, B)
    S.write_kitti_poses(str(tmp_path / "f32.txt"), traj)
    assert open(str(tmp_path / "f32.txt"), "rb").read() != files[0]
    inline = S.kitti_window_loader(dumps["f32"], 3, FRAMES, H, W, flow="f16")(0, 2)
    assert inline[1].dtype == np.float16
    assert S.synthetic_window_loader(H, W, flow="f16")(0, 2)[1].dtype == np.float16


def test_the_drivers_list_the_option():
    out = subprocess.run([sys.executable, "-m", "davo_amd.run_kitti_pose", "--help"], check=True, capture_output=True, text=True, cwd=ROOT).stdout
    assert "--flow {f32,f16}" in out
    for tool in ("config1_stream.py", "config4_from_files.py", "measure_host_api.py"):
        src = open(os.path.join(ROOT, "tools", tool)).read()
        assert "--flow" in src, tool


def test_what_the_opt_in_costs_in_the_poses():
    """A recorded measurement, not a gate: the float64 oracle at 32x64, B = 2, flagship, synthetic inputs and weights, on flow x
    and on flow_from_f16(flow_to_f16(x)).  Measured: the largest change of the 6-DoF outputs is 1.84e-5 at a largest |pose| of
    0.221, 8.3e-5 relative, for a largest flow change of 0.0156 px (half the spacing of the halves between 32 and 64 px).  The
    project's bar for the kernels against the oracle is 1e-4 absolute and relative: the opt-in spends
    most of that margin on these inputs - white-noise flow of 15 px standard deviation, the worst case for a rounding of every
    pixel - which is why it is an opt-in.  INTEGRATION.md quotes the figure.  Printed with -s; asserted only: the rounding
    moves the flow, so it moves the poses."""
    from oracle import c_oracle
    cfg = davo_amd.parse_version(davo_amd.FLAGSHIP_VERSION)
    img, flow, seg = synth.make_inputs(2, 32, 64)
    weights = synth.make_weights(cfg)
    rounded = flow_from_f16(flow_to_f16(flow))
    a, b = c_oracle.forward(cfg, img, flow, seg, weights), c_oracle.forward(cfg, img, rounded, seg, weights)
    change, scale = float(np.abs(a.astype(np.float64) - b).max()), float(np.abs(a).max())
    print("binary16 flow, float64 oracle, 32x64 B=2 flagship: max |pose change| = %.3g at max |pose| = %.3g (relative %.3g); "
          "max |flow change| = %.3g px" % (change, scale, change / scale, float(np.abs(flow - rounded).max())))
    assert np.isfinite(a).all() and np.isfinite(b).all() and change > 0

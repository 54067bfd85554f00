"""Binary16 depth planes without a GPU (include/davo_hip.h: davo_set_depth_format): the one host-side rounding rule and its
widening twin, the C surface, the frame plan's byte counts, the synthetic twins, the loaders, the drivers' option - what the
opt-in costs in the poses, recorded on the float64 restatements - and the preconditions of the GPU cases
(tests/f16_depth_cases.py), checked on the restatements alone.

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
from davo_amd.depth import DEPTH_DTYPES, DEPTH_FORMATS, check_depth_format, depth_from_f16, depth_to_f16
from davo_amd.version import ATT_SOURCE

import f16_depth_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_CODES = {"src0": 1, "src1": 2, "both": 3}


def _all_halves():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def _bits16(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def _one(x):
    return int(_bits16(depth_to_f16(np.float32([x])))[0])


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
        bits = abits if abits % 2 == 0 else bbits            # the tie goes to the even significand
    if bits == 0 and np.signbit(np.float32(x)):
        bits = 0x8000                                        # a result that rounds to zero keeps the sign
    return bits


# ---- the rounding rule ------------------------------------------------------------------------------------------------
def test_the_rule_rounds_to_nearest_even_and_saturates():
    ulp8 = 2.0 ** -7                                         # spacing of the halves in [8, 16): the depth-split threshold's binade
    ties = [8 + ulp8 / 2, 8 + 3 * ulp8 / 2, 15 + ulp8 / 2, -(8 + ulp8 / 2), 2049.0, 2051.0, 65504 - 16.0, 2.0 ** -25, 3 * 2.0 ** -25,
            -(2.0 ** -25), 2.0 ** -24 + 2.0 ** -25, 1023.5 * 2.0 ** -24]
    for v, want in ((8 + ulp8 / 2, 0x4800), (8 + 3 * ulp8 / 2, 0x4802), (2049.0, 0x6800), (2051.0, 0x6802), (2.0 ** -25, 0x0000),
                    (3 * 2.0 ** -25, 0x0002), (-(2.0 ** -25), 0x8000)):
        assert _one(v) == want, v
    rng = np.random.default_rng(20261020)
    values = np.concatenate([np.asarray(ties, np.float32), np.exp2(rng.uniform(0, 6.5, 3000)).astype(np.float32),      # a depth range
                             (rng.uniform(-1, 1, 500) * 2.0 ** -14).astype(np.float32),       # around the subnormal range
                             (rng.uniform(-1, 1, 300) * 2.0 ** -23).astype(np.float32),
                             rng.uniform(-70000, 70000, 500).astype(np.float32),
                             synth.make_depth(1, 16, 24).ravel()])
    got = _bits16(depth_to_f16(values))
    want = np.array([_nearest_even_half(v) for v in values], np.uint16)
    assert np.array_equal(got, want), values[got != want][:5]
    for v in (65504.0, 65519.99, 65520.0, 70000.0, 1e9, 3.4e38):      # the saturation edge: binary16 would round 65520 to infinity
        assert _one(v) == 0x7BFF and _one(-v) == 0xFBFF, v
    assert _one(65503.99) == 0x7BFF and _one(65488.0) == 0x7BFE     # (the tie at 65488 goes to the even 65472)
    assert np.isfinite(depth_to_f16(values)).all()
    sp = depth_to_f16(np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0 ** -24, -1023 * 2.0 ** -24, 1e-30, -1e-30]))
    assert np.isnan(sp[0]) and list(_bits16(sp[1:])) == [0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x83FF, 0x0000, 0x8000]
    shaped = depth_to_f16(np.ones((2, 3, 4, 8, 1), np.float32))
    assert shaped.shape == (2, 3, 4, 8, 1) and shaped.dtype == np.float16
    assert davo_amd.depth_to_f16 is depth_to_f16 and davo_amd.depth_from_f16 is depth_from_f16      # one definition
    # the flow's rule, bit for bit
    assert np.array_equal(_bits16(depth_to_f16(values)), _bits16(davo_amd.flow_to_f16(values)))


def test_rounding_is_an_involution_through_the_widening_on_every_half():
    h = _all_halves()
    w = depth_from_f16(h)
    assert w.dtype == np.float32 and w.shape == h.shape
    nan = np.isnan(h)
    assert nan.sum() == 2 * 1023 and np.isnan(w[nan]).all() and np.isnan(depth_to_f16(w[nan])).all()
    assert np.array_equal(_bits16(depth_to_f16(w))[~nan], _bits16(h)[~nan])       # round(widen(x)) == x: all 65,536 less the NaNs
    bits = _bits16(h).astype(np.int64)
    sign, ex, man = np.where(bits >> 15, -1.0, 1.0), (bits >> 10) & 31, bits & 1023
    value = np.where(ex == 0, man * 2.0 ** -24, (1024 + man) * 2.0 ** (ex.astype(np.float64) - 25))
    fin = ex < 31
    assert np.array_equal(w[fin].astype(np.float64), (sign * value)[fin]) and np.array_equal(np.signbit(w[fin]), bits[fin] >> 15 == 1)
    assert np.array_equal(w[(ex == 31) & (man == 0)], np.float32([np.inf, -np.inf]))
    with pytest.raises(ValueError, match="float16"):
        depth_from_f16(np.zeros(4, np.float32))
    assert DEPTH_FORMATS == {"f32": 0, "f16": 1} and DEPTH_DTYPES["f16"] == np.float16 and check_depth_format("f16") == "f16"
    with pytest.raises(ValueError, match="depth"):
        check_depth_format("half")


# ---- the C surface ----------------------------------------------------------------------------------------------------
def test_surface():
    header = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    assert re.search(r"int davo_set_depth_format\(davo_ctx\* ctx, int fmt\);", header)
    assert re.search(r"int davo_get_depth_format\(const davo_ctx\* ctx\);", header)
    assert re.search(r"DAVO_DEPTH_F32 = 0\b", header) and re.search(r"DAVO_DEPTH_F16 = 1\b", header)
    assert re.search(r"int davo_frames_plan_fmt2\(int H, int W, int N, int pairs, int att_source, int label_fmt, int flow_fmt, int depth_fmt, int\* ranges,\s*long long\* link_bytes\);", header)
    for figure in ("1,650,688", "1,331,200", "1,011,712", "638,976", "319,488", "851,968", "745,472"):      # the byte counts a caller plans with
        assert figure in header, figure
    assert "The depth planes stay float32" not in header
    assert (_lib.DEPTH_F32, _lib.DEPTH_F16) == (0, 1)
    for name in ("davo_set_depth_format", "davo_get_depth_format", "davo_frames_plan_fmt2"):
        assert name in _lib.EXPORTS
    lib = _lib.lib()
    assert lib.davo_set_depth_format.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.davo_get_depth_format.argtypes == [ctypes.c_void_p]
    raw = ctypes.CDLL(_lib.LIB_PATH)                         # the library's own export table, not the binding's list
    assert raw.davo_set_depth_format and raw.davo_get_depth_format and raw.davo_frames_plan_fmt2
    assert lib.davo_set_depth_format(None, 1) == -1 and lib.davo_get_depth_format(None) == -1      # no context: DAVO_ERR_INVALID
    assert callable(davo_amd.Engine.set_depth_format) and callable(davo_amd.DAVO.use_f16_depth)


def _depth_table(N, pairs, att):
    """the header's table ("Frame sequences"), depth column: [lo, hi) of the depth planes a batch of N windows reads"""
    if att not in ("se_depth_wo_tgt_to_seg", "se_depth_to_seg", "se_flow_depthseg_sep"):
        return (0, 0)
    split = att == "se_flow_depthseg_sep"
    if pairs == "both":
        return (0, N + 2)
    if pairs == "src0":
        return (0, N) if split else (0, N + 1)
    return (2, N + 2) if split else (1, N + 2)


def _plan2(H, W, N, code, att, lab, flow, depth):
    r, b = (ctypes.c_int * 8)(), ctypes.c_longlong(0)
    rc = _lib.lib().davo_frames_plan_fmt2(H, W, N, code, att, lab, flow, depth, r, ctypes.byref(b))
    return rc, list(r), b.value


@pytest.mark.parametrize("pairs", ["both", "src0", "src1"])
def test_frames_plan_fmt2_is_the_headers_table(pairs):
    H, W = 128, 416
    lib, code = _lib.lib(), PAIR_CODES[pairs]
    for att, a in sorted(ATT_SOURCE.items(), key=lambda kv: kv[1]):
        for N in (1, 7, 64):
            for lab in (0, 1):
                for flow in (0, 1):
                    r0, b0 = (ctypes.c_int * 8)(), ctypes.c_longlong(0)
                    assert lib.davo_frames_plan_fmt(H, W, N, code, a, lab, flow, r0, ctypes.byref(b0)) == 0
                    rc, r32, b32 = _plan2(H, W, N, code, a, lab, flow, 0)
                    assert rc == 0 and r32 == list(r0) and b32 == b0.value, (att, N, lab, flow)      # DAVO_DEPTH_F32: davo_frames_plan_fmt
                    rc, r16, b16 = _plan2(H, W, N, code, a, lab, flow, 1)
                    assert rc == 0 and r16 == r32
                    dep = tuple(r16[4:6])
                    assert dep == _depth_table(N, pairs, att), (att, N)
                    assert b32 - b16 == 2 * H * W * (dep[1] - dep[0]), (att, N, lab, flow)
                    if flow == 0 and a <= 13:                # davo_frames_plan: both formats float32
                        r1, b1 = (ctypes.c_int * 8)(), ctypes.c_longlong(0)
                        assert lib.davo_frames_plan(H, W, N, code, a, lab, r1, ctypes.byref(b1)) == 0
                        assert list(r1) == r32 and b1.value == b32
            p = frames_plan(H, W, N, pairs, att, "u8", "f16", "f16")
            assert p["depth"] == _depth_table(N, pairs, att) and p["link_bytes"] == _plan2(H, W, N, code, a, 1, 1, 1)[2]
            assert frames_plan(H, W, N, pairs, att, "u8", "f16", "f32") == frames_plan(H, W, N, pairs, att, "u8", "f16")
    assert _plan2(H, W, 4, code, 11, 0, 0, 2)[0] == -1 and _plan2(H, W, 4, code, 11, 0, 0, -1)[0] == -1
    assert lib.davo_frames_plan_fmt2(H, W, 4, code, 11, 0, 0, 1, None, None) == 0
    with pytest.raises(ValueError, match="depth"):
        frames_plan(H, W, 4, depth="bf16")


def test_the_byte_counts_a_caller_plans_with():
    """include/davo_hip.h, per window at 128x416, source 11, both pairs, byte labels, binary16 flow"""
    H, W = 128, 416
    HW = H * W
    strip, flow, labels = 9 * HW, 2 * HW * 2 * 2, 2 * HW
    assert (strip, flow, labels) == (479232, 425984, 106496) and strip + flow + labels == 1011712
    assert 3 * HW * 4 == 638976 and 3 * HW * 2 == 319488
    assert 1011712 + 638976 == 1650688 and 1011712 + 319488 == 1331200                      # the window layout
    att = "se_depth_wo_tgt_to_seg"
    per_window = lambda **kw: (frames_plan(H, W, 1001, "both", att, "u8", "f16", **kw)["link_bytes"] -      # noqa: E731
                               frames_plan(H, W, 1000, "both", att, "u8", "f16", **kw)["link_bytes"])
    assert per_window() == per_window(depth="f32") == 851968 == 638976 + 4 * HW              # the frame layout, long batch
    assert per_window(depth="f16") == 745472 == 638976 + 2 * HW


# ---- synthetic twins --------------------------------------------------------------------------------------------------
def test_synthetic_twins():
    d = synth.make_depth(2, 16, 24, first_window=5)
    h = synth.make_depth(2, 16, 24, first_window=5, fmt="f16")
    assert d.dtype == np.float32 and h.dtype == np.float16 and h.shape == d.shape == (2, 3, 16, 24, 1)
    assert np.array_equal(_bits16(h), _bits16(depth_to_f16(d)))
    assert not np.array_equal(depth_from_f16(h), d) and np.abs(depth_from_f16(h) / d - 1).max() <= 2.0 ** -11
    fr, fr16 = synth.make_frames(5, 16, 24, depth=True), synth.make_frames(5, 16, 24, depth="f16")
    assert fr[3].dtype == np.float32 and fr16[3].dtype == np.float16 and np.array_equal(_bits16(fr16[3]), _bits16(depth_to_f16(fr[3])))
    for k in range(3):
        assert np.array_equal(fr16[k], fr[k])
    win = davo_amd.windows_from_frames(*fr16)                # the conversions keep the dtype
    assert win[3].dtype == np.float16 and np.array_equal(_bits16(win[3][:, 0]), _bits16(fr16[3][:3]))
    assert davo_amd.frames_from_windows(*win)[3].dtype == np.float16
    assert davo_amd.flip_windows(*win)[3].dtype == np.float16 and davo_amd.flip_frames(*fr16)[3].dtype == np.float16
    with pytest.raises(ValueError, match="depth"):
        synth.make_depth(1, 16, 24, fmt="bf16")
    from davo_amd import sequence as S
    assert S.synthetic_window_loader(16, 24, depth="f16")(0, 2)[3].dtype == np.float16
    assert S.synthetic_window_loader(16, 24, depth=True)(0, 2)[3].dtype == np.float32
    assert len(S.synthetic_window_loader(16, 24)(0, 2)) == 3


# ---- loaders ----------------------------------------------------------------------------------------------------------
H, W, FRAMES, B = 16, 24, 9, 3                               # 7 windows: two whole batches and a short one


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """a float32 dump, its binary16-depth twin and the float32 dump of the twin's widened values"""
    out = {}
    for fmt, depth in (("f32", True), ("f16", "f16"), ("widened", "widened")):
        out[fmt] = str(tmp_path_factory.mktemp("ddump_" + fmt))
        for seq, seed in ((3, 11), (4, 12)):
            L.write_synthetic_dump(out[fmt], seq, FRAMES, H, W, seed=seed, depth=depth)
    return out


def test_the_half_dump_is_the_float_dumps_twin(dumps):
    for w in (1, FRAMES - 2):
        a, b, c = (np.load(L.depth_path(dumps[k], 3, w)) for k in ("f32", "f16", "widened"))
        assert a.dtype == np.float32 and b.dtype == np.float16 and c.dtype == np.float32 and a.shape == b.shape == c.shape == (3, H, W, 1)
        assert np.array_equal(_bits16(b), _bits16(depth_to_f16(a))) and np.array_equal(c, depth_from_f16(b))
        for k in range(3):                                   # strips, flow and label maps are the same files
            assert open(L.window_paths(dumps["f32"], 3, w)[k], "rb").read() == open(L.window_paths(dumps["f16"], 3, w)[k], "rb").read()
    with pytest.raises(ValueError, match="depth"):
        L.write_synthetic_dump(dumps["f32"], 9, 3, H, W, depth="bf16")


def _collect(loader):
    return [(s, e, tuple(np.array(p) for p in parts)) for s, e, parts in loader]


def test_threaded_loader(dumps):
    want = _collect(L.kitti_loader(dumps["f32"], 3, H, W, 0, FRAMES - 2, B, workers=2, depth=True))
    assert [(s, e) for s, e, _ in want] == [(0, 3), (3, 6), (6, 7)] and want[0][2][3].dtype == np.float32
    for dump in ("f16", "f32"):                              # read as it is; converted by the worker
        got = _collect(L.kitti_loader(dumps[dump], 3, H, W, 0, FRAMES - 2, B, workers=2, depth="f16"))
        assert len(got) == len(want)
        for (s, e, g), (s0, e0, w) in zip(got, want):
            assert (s, e) == (s0, e0) and g[3].dtype == np.float16 and g[3].shape == w[3].shape
            assert np.array_equal(_bits16(g[3]), _bits16(depth_to_f16(w[3])))
            for k in range(3):
                assert np.array_equal(g[k], w[k])
    one = L.load_window(dumps["f16"], 3, 1, H, W, depth="f16")[3]
    assert one.dtype == np.float16 and np.array_equal(_bits16(one), _bits16(depth_to_f16(L.load_window(dumps["f32"], 3, 1, H, W, depth=True)[3])))
    assert L.load_window(dumps["f32"], 3, 1, H, W, depth="f32")[3].dtype == np.float32 and len(L.load_window(dumps["f32"], 3, 1, H, W)) == 3
    every = L.load_window(dumps["f32"], 3, 1, H, W, depth="f16", labels="u8", flow="f16")
    assert every[1].dtype == np.float16 and every[2].dtype == np.uint8 and every[3].dtype == np.float16


def _process_batches(dump, depth, segments=None, **kw):
    if segments is None:
        ld = L.ProcessWindowLoader(dump, 3, H, W, 0, FRAMES - 2, B, procs=2, depth=depth, **kw)
    else:
        ld = L.ProcessWindowLoader(dump, None, H, W, None, None, B, procs=2, depth=depth, segments=segments, **kw)
    try:
        return [_collect(ld)] if segments is None else [_collect(ld.segment(k)) for k in range(len(segments))]
    finally:
        ld.close()


def test_process_loader(dumps):
    want = _process_batches(dumps["f32"], True)
    for dump in ("f16", "f32"):
        got = _process_batches(dumps[dump], "f16")
        assert [(s, e) for s, e, _ in got[0]] == [(0, 3), (3, 6), (6, 7)]
        for (s, e, g), (_, _, w) in zip(got[0], want[0]):
            assert g[3].dtype == np.float16 and np.array_equal(_bits16(g[3]), _bits16(depth_to_f16(w[3]))), (dump, s)
            for k in range(3):
                assert np.array_equal(g[k], w[k])
    segments = [(3, 0, FRAMES - 2), (4, 2, 6)]               # two segments from one pool, with byte labels and binary16 flow
    want2 = _process_batches(dumps["f32"], True, segments)
    for dump in ("f16", "f32"):
        got2 = _process_batches(dumps[dump], "f16", segments, labels="u8", flow="f16")
        for k in range(2):
            assert [(s, e) for s, e, _ in got2[k]] == [(s, e) for s, e, _ in want2[k]]
            for (_, _, g), (_, _, w) in zip(got2[k], want2[k]):
                assert np.array_equal(_bits16(g[3]), _bits16(depth_to_f16(w[3]))) and g[1].dtype == np.float16 and g[2].dtype == np.uint8


def test_process_loader_depth_segments_hold_half_the_bytes(dumps):
    sizes = {}
    for fmt, depth in (("f32", True), ("f16", "f16")):
        ld = L.ProcessWindowLoader(dumps["f32"], 3, H, W, 0, FRAMES - 2, B, procs=1, depth=depth)
        ld.start()
        try:
            sizes[fmt] = [v[3].nbytes for v in ld._views]
            assert all(v[3].dtype == DEPTH_DTYPES[fmt] for v in ld._views)
            assert all(quad[3].size >= v[3].nbytes for quad, v in zip(ld._segs, ld._views))
            assert all(quad[3].size < 2 * v[3].nbytes for quad, v in zip(ld._segs, ld._views)) or fmt == "f32"
        finally:
            ld.close()
    assert len(sizes["f16"]) == len(sizes["f32"]) > 0
    assert all(2 * a == b == B * 3 * H * W * 4 for a, b in zip(sizes["f16"], sizes["f32"]))


def test_any_other_depth_dtype_is_an_error_that_names_the_file(dumps, tmp_path):
    bad = str(tmp_path / "bad")
    shutil.copytree(dumps["f32"], bad)
    path = L.depth_path(bad, 3, 2)
    np.save(path, np.load(path).astype(np.float64))
    with pytest.raises(ValueError, match=re.escape(path)):
        L.load_window(bad, 3, 2, H, W, depth="f16")
    with pytest.raises(ValueError, match=re.escape(path)):
        _collect(L.kitti_loader(bad, 3, H, W, 0, FRAMES - 2, B, workers=2, depth="f16"))
    with pytest.raises(ValueError, match=re.escape(path)):
        _process_batches(bad, "f16")
    with pytest.raises(ValueError, match="depth"):
        L.kitti_loader(dumps["f32"], 3, H, W, 0, 1, B, depth="half")
    with pytest.raises(ValueError, match="depth"):
        L.ProcessWindowLoader(dumps["f32"], 3, H, W, 0, 1, B, depth="half")
    with pytest.raises(ValueError, match="depth slot"):
        L.load_window_into(dumps["f32"], 3, 1, H, W, np.empty((H, 3 * W, 3), np.uint8), np.empty((4, H, W, 2), np.float32),
                           np.empty((3, H, W, 1), np.float32), depth=np.empty((3, H, W, 1), np.float64))


def test_the_sequence_loaders_carry_the_format(dumps):
    from davo_amd import sequence as S
    inline = S.kitti_window_loader(dumps["f32"], 3, FRAMES, H, W, depth="f16")(0, 2)
    assert len(inline) == 4 and inline[3].dtype == np.float16
    assert np.array_equal(_bits16(inline[3]), _bits16(depth_to_f16(S.kitti_window_loader(dumps["f32"], 3, FRAMES, H, W, depth=True)(0, 2)[3])))
    ld = S.kitti_window_loader(dumps["f16"], 3, FRAMES, H, W, workers=2, depth="f16")
    parts = next(iter(ld.for_range(0, FRAMES - 2, B)))[2]
    assert parts[3].dtype == np.float16


def test_the_drivers_list_the_option():
    for module in ("davo_amd.run_kitti_pose", "davo_amd.generate_feature_map"):
        out = subprocess.run([sys.executable, "-m", module, "--help"], check=True, capture_output=True, text=True, cwd=ROOT).stdout
        assert "--depth {f32,f16}" in out, module
    assert "--depth" in open(os.path.join(ROOT, "tools", "variant_step.py")).read()


# ---- what the opt-in costs, and why the GPU cases can tell ------------------------------------------------------------
def _recorded_costs():
    """the three maxima INTEGRATION.md quotes, from its "Depth planes as binary16" section"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("Depth planes as binary16"):]
    out = {}
    for source in C.SOURCES:
        m = re.search(r"source %d[^|]*\|\s*([0-9.]+e[-+][0-9]+)\s*\|" % source, section)
        assert m, source
        out[source] = float(m.group(1))
    return out


def test_what_the_opt_in_costs_in_the_poses():
    """The float64 restatements at 36x100, B = 3, on synth inputs, d against depth_from_f16(depth_to_f16(d)); the largest change
    of the 6-DoF outputs per source is recorded in INTEGRATION.md.  Sources 11 and 12 see the rounding through the mean of a
    plane, where 3600 roundings of either sign average out.  Source 13's case places the threshold on a half's value, so every
    pixel that rounds onto it changes side: the worst placement, and the figure is its price.  The computation is deterministic;
    the factor 2 is for numpy's summation order alone."""
    recorded = _recorded_costs()
    for source in C.SOURCES:
        c = C.case(source, *C.COST_SHAPE)
        change = C.preconditions(c, None)
        print("binary16 depth, float64 restatement, source %d at %dx%d B=%d: max |pose change| = %.6g (recorded %.6g)"
              % ((source,) + C.COST_SHAPE + (change, recorded[source])))
        assert change > 0
        assert recorded[source] / 2 <= change <= recorded[source] * 2, (source, change, recorded[source])


@pytest.mark.parametrize("shape", C.SHAPES, ids=["%dx%d" % s[:2] for s in C.SHAPES])
@pytest.mark.parametrize("source", C.SOURCES)
def test_preconditions_of_the_gpu_cases(source, shape):
    """In every case's inputs the rounding moves most pixels, source 13's threshold separates some pixel's float32 depth from its
    rounded one with both sides populated, and the restatement's poses on d and on the widened halves differ in at least one bit:
    a library that read other values than the halves' could not agree with a float32 engine on the widened halves."""
    assert C.preconditions(C.case(source, *shape), None) > 0


@pytest.mark.parametrize("N,H,W", C.FRAME_CASES, ids=["N%d" % f[0] for f in C.FRAME_CASES])
@pytest.mark.parametrize("source", C.SOURCES)
def test_preconditions_of_the_frame_layout_cases(source, N, H, W):
    """the same on the windows that the frame-layout cases' frames expand to"""
    c, fr = C.frames_case(source, N, H, W)
    assert fr[4].dtype == np.float16 and fr[4].shape == (N + 2, H, W, 1) and np.array_equal(_bits16(fr[4]), _bits16(depth_to_f16(fr[3])))
    assert np.array_equal(_bits16(c.h), _bits16(davo_amd.windows_from_frames(fr[0], fr[1], fr[2], fr[4])[3]))
    assert C.preconditions(c, None) > 0

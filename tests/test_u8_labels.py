"""Byte label maps without a GPU (include/davo_hip.h: davo_set_label_format): the one host-side rule, the C surface, the loaders,
the synthetic inputs and the driver's option.

The rule is checked against a restatement of the kernels' att_lookup (csrc/input_decode.h): for every float the class the float
selects - a finite value in (-1, 19) selects row int(value), truncated toward zero; anything else selects none - must be the
class the byte selects on the device - row L when L < 19, none otherwise."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import davo_amd
from davo_amd import _lib, loader as L, synth
from davo_amd.labels import labels_to_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _class_of_float(x):
    """att_lookup's rule, one value at a time in Python arithmetic: the selected row, or -1"""
    x = float(np.float32(x))
    if x != x or not (x > -1.0 and x < 19.0):
        return -1
    return int(x)                                            # truncates toward zero


def _class_of_byte(b):
    return int(b) if int(b) < 19 else -1


SPECIAL = [-1.0, -0.999, -0.5, -0.0, 0.0, 0.99, 5.5, 18.0, 18.9, 19.0, 200.0, 255.0, 256.0, 3e9, -3e9, np.inf, -np.inf, np.nan]


def test_the_rule_selects_the_class_the_float_selects():
    rng = np.random.default_rng(20261019)
    values = np.concatenate([np.asarray(SPECIAL, np.float32), rng.uniform(-3.0, 25.0, 100000).astype(np.float32)])
    got = labels_to_u8(values)
    assert got.dtype == np.uint8 and got.shape == values.shape
    want = np.array([_class_of_float(v) for v in values])
    sel = np.array([_class_of_byte(b) for b in got])
    assert np.array_equal(sel, want)
    assert (got[want < 0] == 255).all()                      # everything that is no class becomes 255, Cityscapes' ignore label
    for v, b in ((-0.5, 0), (-0.0, 0), (18.9, 18), (-1.0, 255), (19.0, 255), (255.0, 255), (np.nan, 255), (np.inf, 255), (-3e9, 255)):
        assert labels_to_u8(np.float32(v)) == b, v
    k = np.arange(19)
    assert np.array_equal(labels_to_u8(k.astype(np.float32)), k)
    shaped = labels_to_u8(np.zeros((2, 3, 4, 8, 1), np.float32))
    assert shaped.shape == (2, 3, 4, 8, 1)
    assert davo_amd.labels_to_u8 is labels_to_u8             # one definition


def test_surface():
    header = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    assert re.search(r"int davo_set_label_format\(davo_ctx\* ctx, int fmt\);", header)
    assert re.search(r"int davo_get_label_format\(const davo_ctx\* ctx\);", header)
    assert re.search(r"DAVO_LABELS_F32 = 0\b", header) and re.search(r"DAVO_LABELS_U8 = 1\b", header)
    assert (_lib.LABELS_F32, _lib.LABELS_U8) == (0, 1)
    assert "davo_set_label_format" in _lib.EXPORTS and "davo_get_label_format" in _lib.EXPORTS
    lib = _lib.lib()
    assert lib.davo_set_label_format.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.davo_get_label_format.argtypes == [ctypes.c_void_p]
    raw = ctypes.CDLL(_lib.LIB_PATH)                         # the library's own export table, not the binding's list
    assert raw.davo_set_label_format and raw.davo_get_label_format
    assert ctypes.sizeof(_lib.DavoVariant) == 32             # the variant is still eight ints
    assert lib.davo_set_label_format(None, 1) == -1 and lib.davo_get_label_format(None) == -1      # no context: DAVO_ERR_INVALID


def test_synthetic_inputs():
    img, flow, seg = synth.make_inputs(2, 16, 24, first_window=5)
    img8, flow8, seg8 = synth.make_inputs(2, 16, 24, first_window=5, labels="u8")
    assert seg8.dtype == np.uint8 and seg8.shape == seg.shape
    assert np.array_equal(seg8, labels_to_u8(seg)) and np.array_equal(img8, img) and np.array_equal(flow8, flow)
    assert (seg8 == 255).any() and (seg8 < 19).any()
    with pytest.raises(ValueError, match="labels"):
        synth.make_inputs(1, 16, 24, labels="u16")


H, W, FRAMES, B = 16, 24, 9, 3                               # 7 windows: two whole batches and a short one


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """a float dump and its byte twin, two sequences each"""
    f32, u8 = str(tmp_path_factory.mktemp("dump_f32")), str(tmp_path_factory.mktemp("dump_u8"))
    for seq, seed in ((3, 11), (4, 12)):
        L.write_synthetic_dump(f32, seq, FRAMES, H, W, seed=seed)
        L.write_synthetic_dump(u8, seq, FRAMES, H, W, seed=seed, labels="u8")
    return f32, u8


def test_the_byte_dump_is_the_float_dumps_twin(dumps):
    f32, u8 = dumps
    for w in (1, FRAMES - 2):
        a, b = np.load(L.window_paths(f32, 3, w)[2]), np.load(L.window_paths(u8, 3, w)[2])
        assert a.dtype == np.float32 and b.dtype == np.uint8 and b.shape == a.shape == (3, H, W, 1)
        assert np.array_equal(b, labels_to_u8(a))
        for k in (0, 1):                                     # strips and flow are the same files
            assert open(L.window_paths(f32, 3, w)[k], "rb").read() == open(L.window_paths(u8, 3, w)[k], "rb").read()


def _collect(loader):
    out = []
    for s, e, parts in loader:
        out.append((s, e, tuple(np.array(p) for p in parts)))
    return out


def test_threaded_loader(dumps):
    f32, u8 = dumps
    want = _collect(L.kitti_loader(f32, 3, H, W, 0, FRAMES - 2, B, workers=2))
    assert [(s, e) for s, e, _ in want] == [(0, 3), (3, 6), (6, 7)] and want[0][2][2].dtype == np.float32
    for dump in (f32, u8):
        got = _collect(L.kitti_loader(dump, 3, H, W, 0, FRAMES - 2, B, workers=2, labels="u8"))
        assert len(got) == len(want)
        for (s, e, g), (s0, e0, w) in zip(got, want):
            assert (s, e) == (s0, e0) and g[2].dtype == np.uint8 and g[2].shape == w[2].shape
            assert np.array_equal(g[2], labels_to_u8(w[2])) and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
    one = L.load_window(u8, 3, 1, H, W, labels="u8")[2]
    assert one.dtype == np.uint8 and np.array_equal(one, labels_to_u8(L.load_window(f32, 3, 1, H, W)[2]))


def _process_batches(dump, labels, segments=None, seg_planes=L.SEG_PLANES_SOURCES):
    """the batches of one range (sequence 3, every window), or of every segment of ``segments``: [[(s, e, parts), ...], ...]"""
    if segments is None:
        ld = L.ProcessWindowLoader(dump, 3, H, W, 0, FRAMES - 2, B, procs=2, seg_planes=seg_planes, labels=labels)
    else:
        ld = L.ProcessWindowLoader(dump, None, H, W, None, None, B, procs=2, seg_planes=seg_planes, labels=labels, segments=segments)
    try:
        return [_collect(ld)] if segments is None else [_collect(ld.segment(k)) for k in range(len(segments))]
    finally:
        ld.close()


def test_process_loader(dumps):
    f32, u8 = dumps
    want = _process_batches(f32, "f32")
    for dump in (f32, u8):
        got = _process_batches(dump, "u8")
        assert [(s, e) for s, e, _ in got[0]] == [(0, 3), (3, 6), (6, 7)]                 # whole batches and a short last one
        for (s, e, g), (_, _, w) in zip(got[0], want[0]):
            assert g[2].dtype == np.uint8 and np.array_equal(g[2], labels_to_u8(w[2])), (dump, s)
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
            assert (g[2][:, 1] == 0).all()                   # seg_planes of the sources alone: the target's plane is never read
    # every plane, and two segments from one pool
    segments = [(3, 0, FRAMES - 2), (4, 2, 6)]
    want2 = _process_batches(f32, "f32", segments, seg_planes=(0, 1, 2))
    for dump in (f32, u8):
        got2 = _process_batches(dump, "u8", segments, seg_planes=(0, 1, 2))
        for k in range(2):
            assert [(s, e) for s, e, _ in got2[k]] == [(s, e) for s, e, _ in want2[k]]
            for (_, _, g), (_, _, w) in zip(got2[k], want2[k]):
                assert np.array_equal(g[2], labels_to_u8(w[2])) and g[2][:, 1].any()


def test_process_loader_label_segments_hold_a_quarter_of_the_bytes(dumps):
    f32, _ = dumps
    sizes = {}
    for labels in ("f32", "u8"):
        ld = L.ProcessWindowLoader(f32, 3, H, W, 0, FRAMES - 2, B, procs=1, labels=labels)
        ld.start()
        try:
            sizes[labels] = [v[2].nbytes for v in ld._views]
            assert all(v[2].dtype == L.LABEL_DTYPES[labels] for v in ld._views)
            assert all(trio[2].size >= v[2].nbytes for trio, v in zip(ld._segs, ld._views))
        finally:
            ld.close()
    assert len(sizes["u8"]) == len(sizes["f32"]) > 0
    assert all(4 * a == b == B * 3 * H * W * 4 for a, b in zip(sizes["u8"], sizes["f32"]))


def test_any_other_label_dtype_is_an_error_that_names_the_file(dumps, tmp_path):
    f32, _ = dumps
    import shutil
    bad = str(tmp_path / "bad")
    shutil.copytree(f32, bad)
    path = L.window_paths(bad, 3, 2)[2]
    np.save(path, np.load(path).astype(np.int32))
    with pytest.raises(ValueError, match=re.escape(path)):
        L.load_window(bad, 3, 2, H, W, labels="u8")
    with pytest.raises(ValueError, match=re.escape(path)):
        _collect(L.kitti_loader(bad, 3, H, W, 0, FRAMES - 2, B, workers=2, labels="u8"))
    with pytest.raises(ValueError, match=re.escape(path)):
        _process_batches(bad, "u8")
    with pytest.raises(ValueError, match="labels"):
        L.kitti_loader(f32, 3, H, W, 0, 1, B, labels="bytes")
    with pytest.raises(ValueError, match="label slot"):      # a float slot handed over as a byte one
        L.load_window_into(f32, 3, 1, H, W, np.empty((H, 3 * W, 3), np.uint8), np.empty((4, H, W, 2), np.float32),
                           np.empty((3, H, W, 1), np.float32), labels="u8")


def test_the_drivers_list_the_option():
    for module in ("davo_amd.run_kitti_pose", "davo_amd.generate_feature_map"):
        out = subprocess.run([sys.executable, "-m", module, "--help"], check=True, capture_output=True, text=True, cwd=ROOT).stdout
        assert "--labels {f32,u8}" in out, module

"""Class-sorted GEMM rows on the GPU ("pad_classes", csrc/pad_classes.h, csrc/conv_igemm.h: conv_igemm_f32_pc): float32 cnv4, cnv5
and cnv6 on rows sorted by padding class, each tile walking only the taps that are real for its own pixels.  The dropped terms
are exact zeros and every other term of an output's fma chain keeps its place, so the activations and the poses equal the
natural order's to the bit (np.array_equal: a dropped zero term can only turn a +0 into a -0, which compare equal, and ReLU
follows)."""
import numpy as np
import pytest

from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION

from helpers import assert_pose_close

pytestmark = pytest.mark.gpu

LAYERS = (("cnv4", 128), ("cnv5", 256), ("cnv6", 256))
RATES = {"cnv4": 4, "cnv5": 8, "cnv6": 2}


def sorted_layers(H, W, B):
    """the layers that get class-sorted tables at this shape (davo_pad_class_tables returns 1); the others keep the natural order
    and the kernel without tables, because sorting would walk no fewer taps there"""
    import ctypes
    from davo_amd import _lib
    L = _lib.lib()
    Ho, Wo, NB = H // 4, W // 4, 2 * B
    mt = -(-NB * Ho * Wo // 128)
    rows, taps = np.zeros(mt * 128, np.int32), np.zeros(mt, np.uint16)
    out = set()
    for name, rate in RATES.items():
        rc = L.davo_pad_class_tables(NB, Ho, Wo, Ho, Wo, rate, rate, rate, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                     taps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
        assert rc in (0, 1)
        if rc:
            out.add(name)
    return out


def _run(e, img, flow, seg, H, W, B):
    poses = e.forward(img, flow, seg)
    acts = {name: e.debug_read(name, (2 * B, H // 4, W // 4, ch)) for name, ch in LAYERS}
    return poses, acts


@pytest.mark.parametrize("H,W,B,expect", [
    # 8-row maps, one image per block: every class is smaller than a tile, sorting walks no fewer taps, all three layers keep the
    # natural order and the kernel without tables - the option must change nothing
    (32, 416, 4, set()),
    # odd image count (18 pair images, blocks of 3): tiles straddle images and blocks, the last tile ends in -1 rows
    (128, 416, 9, {"cnv4", "cnv5", "cnv6"}),
    # a 16x208 map: rates 4 and 8 sort, rate 2 (classes of two columns) keeps the natural order
    (64, 832, 8, {"cnv4", "cnv5"}),
])
def test_bit_identical_to_the_natural_order(c_oracle, H, W, B, expect):
    assert sorted_layers(H, W, B) == expect          # which kernels the cases below run is known, not hoped for
    cfg = parse_version(FLAGSHIP_VERSION)
    img, flow, seg = synth.make_inputs(B, H, W, first_window=3)
    weights = synth.make_weights(cfg)
    e = Engine(cfg, H, W, B)
    e.load_weights(weights)
    e.set_precision("f32")
    got = {}
    for pc in (1, 0):
        e.set_option("pad_classes", 15 if pc else 0)          # 8 + 7: all three layers, cnv4 too (not in the default set)
        got[pc] = _run(e, img, flow, seg, H, W, B)
    for name, _ in LAYERS:
        assert np.array_equal(got[0][1][name], got[1][1][name]), name
    assert np.array_equal(got[0][0], got[1][0])
    e.close()
    assert_pose_close(got[1][0], c_oracle.forward(cfg, img, flow, seg, weights), "%dx%d B=%d pad_classes" % (H, W, B))


def test_bit_identical_on_the_merged_grid_at_batch_32(c_oracle):
    """B = 32 at 128x416, eight windows tiled four times: cnv4, cnv5 and cnv6 run as merged main + remainder grids.  Natural order
    and class-sorted rows agree to the bit, so do the four copies of the windows (other blocks, other tiles, other launches of
    the grid) and the two ways of handing out the tiles ("skip_order")."""
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 32, 128, 416
    assert sorted_layers(H, W, B) == {"cnv4", "cnv5", "cnv6"}
    img8, flow8, seg8 = synth.make_inputs(8, H, W, first_window=40)
    img, flow, seg = np.tile(img8, (4, 1, 1, 1)), np.tile(flow8, (4, 1, 1, 1, 1)), np.tile(seg8, (4, 1, 1, 1, 1))
    weights = synth.make_weights(cfg)
    e = Engine(cfg, H, W, B)
    e.load_weights(weights)
    e.set_precision("f32")
    e.set_option("host_chunk", 0)            # the whole batch as one piece: the launch plan of a resident batch of 32
    e.set_option("pad_classes", 15)          # 8 + 7: all three layers, cnv4 too (not in the default set)
    p1, a1 = _run(e, img, flow, seg, H, W, B)
    assert len(e.last_plan(4)) == 1 and e.last_plan(4)[0][0] == 2 * B * 32 * 104 // 128        # one grid covers cnv5
    for name, _ in LAYERS:
        for r in range(1, 4):
            assert np.array_equal(a1[name][:16], a1[name][16 * r:16 * r + 16]), (name, r)
    # the poses of the copies: with the pose head on its own (cnv7 stored, every image summed in one fixed order).  Fused into
    # cnv7's epilogue it adds a tile's channels in the tile's own order, and cnv7's two launches have tiles of 128 and of 32
    # columns: copies that land in different launches then differ in the last bit, whatever cnv4..cnv6 ran on
    e.set_option("fuse_pose", 0)
    pu = e.forward(img, flow, seg)
    e.set_option("fuse_pose", 1)
    for r in range(1, 4):
        assert np.array_equal(pu[:8], pu[8 * r:8 * r + 8]), r
    e.set_option("skip_order", 0)
    p1n, a1n = _run(e, img, flow, seg, H, W, B)
    e.set_option("skip_order", 1)
    e.set_option("pad_classes", 0)
    p0, a0 = _run(e, img, flow, seg, H, W, B)
    e.set_option("pad_classes", 1)           # the default set of layers
    pd = e.forward(img, flow, seg)
    e.close()
    assert np.array_equal(pd, p0)
    for name, _ in LAYERS:
        assert np.array_equal(a0[name], a1[name]), name
        assert np.array_equal(a1n[name], a1[name]), name
    assert np.array_equal(p0, p1) and np.array_equal(p1n, p1)
    assert_pose_close(p1[:8], c_oracle.forward(cfg, img8, flow8, seg8, weights), "B=32 pad_classes")

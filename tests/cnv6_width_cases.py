"""The cnv6 widths beside the flagship's 128 (-cnv6_32, -cnv6_64, -cnv6_256) and, per width, the batch sizes at which cnv6
takes each launch plan the planner has for it.  Imported by the tests like layer_check.py: tests/test_cnv6_widths.py keeps the
table complete against davo_plan_layer on the CPU, tests/test_cnv6_widths_gpu.py runs every case layer by layer.

cnv6 is one GEMM of M = 2 B (H / 4) (W / 4) rows and N = 2 x width columns (the rotation and the translation head side by
side): N = 64, 128 or 512 where the flagship has 256, so none of these plans is one the flagship's tests launch."""
from davo_amd import parse_version

WIDTHS = (32, 64, 256)

# plan.h's tile ids by (rows, columns), as davo_plan_layer reports a tile and Engine.last_plan names it
TILE_ID = {(128, 32): 0, (256, 64): 1, (256, 128): 2, (128, 256): 3, (128, 128): 4, (256, 256): 5}

# width -> [(H, W, B, cnv6's tiles: main launch[, remainder launch])].  The smallest B of each tuple at 128x416, then B = 32;
# B = 1, 2, 5 and 32 at every width (the GPU module's launch-option cases run there).  Width 64 at B = 112 is the one batch
# size at 128x416 whose [256x128, 128x128] plan has the shape of the merged main + remainder grid (whole eighths of main
# tiles, 64..256 remainder tiles), which cnv6 must not take: that grid's 256x128 main tile exists for cnv4 alone
# (launch_h3.hip); 256x832 at B = 28 is the first such batch size there.
CASES = {
    32: [(128, 416, 1, (0,)), (128, 416, 2, (0,)), (128, 416, 5, (1,)), (128, 416, 20, (1, 0)), (128, 416, 32, (1,))],
    64: [(128, 416, 1, (0,)), (128, 416, 2, (4,)), (128, 416, 5, (2,)), (128, 416, 10, (2, 0)), (128, 416, 71, (2, 4)),
         (128, 416, 112, (2, 4)), (128, 416, 32, (4,)), (256, 832, 28, (2, 4))],
    256: [(128, 416, 1, (4,)), (128, 416, 2, (2,)), (128, 416, 4, (5,)), (128, 416, 5, (5, 0)), (128, 416, 6, (5, 4)),
          (128, 416, 7, (5, 2)), (128, 416, 32, (5, 2))],
}

# Split-K (forward.hip): cnv6 as one launch of at most SPLIT_K_MAX_TILES tiles runs as 2 or 4 parts over K into float32
# partial sums of parts x N columns.  At 128x416 that is width 32 at B = 1 alone (104 tiles; widths 64 and 256 have 208), so
# each width also runs on two small ragged maps: (H, W, B, cnv6's tiles, M tiles x N tiles).  An image is 225 (36x100) or
# 559 (52x172) rows there, so 128-row tiles straddle images and the last one is cut short (M = 900, 2236).
SPLIT_K_MAX_TILES = 128         # tiles * 2 <= the 256 CUs
SPLIT_K_CASES = {
    32: [(36, 100, 2, (0,), 8 * 2), (52, 172, 2, (0,), 18 * 2)],
    64: [(36, 100, 2, (0,), 8 * 4), (52, 172, 2, (0,), 18 * 4)],
    256: [(36, 100, 2, (0,), 8 * 16), (52, 172, 2, (4,), 18 * 4)],
}

# the batch sizes the table must cover: every tuple the planner emits for a width in these ranges has a case above
COVERED = [(128, 416, range(1, 129)), (256, 832, range(1, 33))]


def version(width):
    return "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_%d-segmask_all-se_flow-abs_flow-fc_tanh" % width


def config(width):
    return parse_version(version(width))


def cnv6_gemm(width, H, W, B):
    """(M, N) of cnv6: the map is the input's size over 4, rounded up (two stride-2 layers, SAME padding)."""
    return 2 * B * (-(-H // 4)) * (-(-W // 4)), 2 * width


def launch_tiles(M, N, tile):
    """Workgroups of one launch of `tile' (a TILE_ID value) over an M x N GEMM."""
    bm, bn = next(k for k, v in TILE_ID.items() if v == tile)
    return -(-M // bm) * (N // bn)


def case_id(width, H, W, B):
    return "cnv6_%d-%dx%d-B%d" % (width, H, W, B)


def cases():
    """[(width, H, W, B, tiles)] of the whole table."""
    return [(w,) + c for w in WIDTHS for c in CASES[w]]


def case(width, B, H=128, W=416):
    for h, w, b, tiles in CASES[width]:
        if (h, w, b) == (H, W, B):
            return tiles
    raise KeyError((width, H, W, B))

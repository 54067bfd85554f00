"""The case table of tests/cnv6_width_cases.py against the planner (davo_plan_layer: host logic, no GPU).  For cnv6 at the
widths 32, 64 and 256 that call is the planner the forward uses: N = 2 x width is never 256, so the 208-pixel tile is not
offered and the efficiencies are not rescaled (forward.hip, allow_208 and others_scale).  Every tile tuple it emits over
B = 1..128 at 128x416 and B = 1..32 at 256x832 must have a GPU case; no tuple is exempt."""
import ctypes

import pytest

from test_abi import built      # noqa: F401  (the module's fixture: builds the library where it is missing)

import cnv6_width_cases as CW


def _planner(path):
    L = ctypes.CDLL(path)
    L.davo_plan_layer.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3

    def plan(M, N):
        rows, bm, bn = (ctypes.c_int * 2)(), (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
        n = L.davo_plan_layer(M, N, 1, rows, bm, bn)
        assert n in (1, 2), (M, N, n)
        return tuple(CW.TILE_ID[(bm[i], bn[i])] for i in range(n))
    return plan


def uncovered(plan, table):
    """[(width, H, W, B, tiles)]: for each tile tuple the planner emits in CW.COVERED and `table' does not list for that
    width, the first batch size that takes it."""
    out = []
    for width in CW.WIDTHS:
        listed = {tiles for _, _, _, tiles in table[width]}
        for H, W, batches in CW.COVERED:
            for B in batches:
                tiles = plan(*CW.cnv6_gemm(width, H, W, B))
                if tiles not in listed:
                    listed.add(tiles)
                    out.append((width, H, W, B, tiles))
    return out


def test_every_cnv6_plan_of_the_other_widths_has_a_gpu_case(built):      # noqa: F811
    missing = uncovered(_planner(built), CW.CASES)
    assert not missing, "cnv6 plans without a case in tests/cnv6_width_cases.py (width, H, W, first B, tiles): %s" % missing


def test_the_table_lists_the_planners_own_tuples(built):      # noqa: F811
    """Each case's tuple is what the planner gives at that case's batch size (a stale entry would send the GPU test after
    a plan that no longer exists), and the cases asked for by name are there."""
    plan = _planner(built)
    for width, H, W, B, tiles in CW.cases():
        assert plan(*CW.cnv6_gemm(width, H, W, B)) == tuple(tiles), CW.case_id(width, H, W, B)
    for width in CW.WIDTHS:
        assert CW.case(width, 32) is not None
        assert len({(H, W, B) for H, W, B, _ in CW.CASES[width]}) == len(CW.CASES[width])
    assert CW.case(64, 112) == (2, 4)


def test_the_split_k_cases_are_launches_that_split(built):      # noqa: F811
    """CW.SPLIT_K_CASES: the planner's tuple is one launch of the tile count listed, which is within forward.hip's bound
    for split-K; and at 128x416 B = 1, where the launch-option cases run, only width 32 is."""
    plan = _planner(built)
    for width in CW.WIDTHS:
        for H, W, B, tiles, count in CW.SPLIT_K_CASES[width]:
            M, N = CW.cnv6_gemm(width, H, W, B)
            assert plan(M, N) == tiles and len(tiles) == 1, (width, H, W, B, plan(M, N))
            assert CW.launch_tiles(M, N, tiles[0]) == count <= CW.SPLIT_K_MAX_TILES, (width, H, W, B)
            assert M % 128 and M // (2 * B) % 128, (width, H, W, B)        # a cut last tile; tiles that straddle images
        M, N = CW.cnv6_gemm(width, 128, 416, 1)
        assert (CW.launch_tiles(M, N, CW.case(width, 1)[0]) <= CW.SPLIT_K_MAX_TILES) == (width == 32)


def test_an_incomplete_table_is_named(built):      # noqa: F811
    """The coverage check itself: with one case taken out, the tuple that lost its case is reported with its width and the
    first batch size that takes it."""
    table = {w: list(c) for w, c in CW.CASES.items()}
    table[256] = [c for c in table[256] if c[3] != (5, 0)]
    assert uncovered(_planner(built), table) == [(256, 128, 416, 5, (5, 0))]


@pytest.mark.parametrize("width", CW.WIDTHS)
def test_versions_parse(width):
    cfg = CW.config(width)
    assert cfg.cnv6_out == width and cfg.att_source == "se_flow"

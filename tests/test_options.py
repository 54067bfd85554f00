"""The launch options as one table (csrc/options.h) through davo_option_info and davo_option_store, on the CPU: the rows, their
defaults, and what davo_set_option stores for a caller's value at every boundary of every rule.  The expected values are typed out
here from include/davo_hip.h's description of the options, not read back from the library."""
import pytest

from davo_amd import _lib

# (name, default in stored form), in the positional order of davo_decide_layer's options 0..13, then davo_decide_forward's 0..6
TABLE = (("wave128", 2), ("skip_order", 1), ("merge_order", -1), ("pad_classes", 6), ("merge_rem_f32", 1), ("share_taps", 1),
         ("merge_rem", 1), ("merge_cnv4", 0), ("tile_208x128", 0), ("deep_ring", 1), ("split_k", 1), ("fold_fixup", 0), ("f32_n16", 1),
         ("f32_n256", 0), ("fold_tails", -1), ("fuse_pack", -1), ("fuse_pose", 1), ("patch_cnv1_t", 1), ("patch_cnv2", 1),
         ("patch_cnv3", 1), ("patch_f32", 1))
SWITCHES = ("share_taps", "merge_rem", "deep_ring", "split_k", "f32_n16", "fuse_pose", "patch_cnv1_t", "patch_cnv2", "patch_cnv3", "patch_f32",
            "merge_cnv4", "tile_208x128", "fold_fixup", "f32_n256")
CLAMPED = {"wave128": (0, 3), "skip_order": (0, 2), "merge_rem_f32": (0, 2)}
# caller's value -> stored value; None = refused
STORED = {
    "merge_order": {-5: -1, -1: -1, 0: 0, 1: 1, 2: 2, 3: 0, 9: 0},
    "fold_tails": {-5: -1, -1: -1, 0: 0, 1: 1, 2: 2, 3: 1, 9: 1},
    "fuse_pack": {-2: -1, -1: -1, 0: 0, 1: 1, 5: 1},
    "pad_classes": {0: 0, 1: 6, 2: None, 7: None, 8: 0, 9: 1, 14: 6, 15: 7, 16: None, -1: None},
}
STORED.update({k: {-1: 1, 0: 0, 1: 1, 2: 1} for k in SWITCHES})
STORED.update({k: dict([(lo - 1, lo), (hi + 1, hi), (-100, lo), (100, hi)] + [(v, v) for v in range(lo, hi + 1)]) for k, (lo, hi) in CLAMPED.items()})
SIDE_EFFECT_KEYS = ("auto_range", "stable_inputs", "force_tile", "cu_partition", "profile_stride", "host_chunk")


def test_the_table_has_these_rows_and_no_more():
    rows = _lib.option_table()
    assert len(rows) == 21 and len({name for name, _ in rows}) == 21
    assert tuple(rows) == TABLE
    L = _lib.lib()
    assert L.davo_option_info(-1, None, None) < 0 and L.davo_option_info(21, None, None) < 0 and L.davo_option_info(20, None, None) == 0


def test_every_row_has_its_rule_here():
    assert set(STORED) == {name for name, _ in TABLE}


@pytest.mark.parametrize("key", [name for name, _ in TABLE])
def test_stored_values(key):
    for value, want in STORED[key].items():
        assert _lib.option_store(key, value) == want, (key, value)
    default = dict(TABLE)[key]                                   # a default is a fixed point of its rule (pad_classes': as 8 + mask)
    assert _lib.option_store(key, 8 + default if key == "pad_classes" else default) == default


def test_keys_that_are_no_launch_options_are_refused():
    for key in SIDE_EFFECT_KEYS + ("no_such_option", "", "wave128 "):
        assert _lib.option_store(key, 1) is None, key
    assert _lib.lib().davo_option_store(None, 1, None) < 0

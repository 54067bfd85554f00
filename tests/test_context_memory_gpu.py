"""What a context allocates goes with it, and scratch that grows changes no result (csrc/owned.h, csrc/ctx.h).

Everything a context allocates is a member that frees itself.  What this file can see of that is device memory, through
hipMemGetInfo: one engine lifetime that touches every lazily built resource must leave exactly the free device bytes the lifetime
before it left (a leaked page-locked block, stream or event, or a table below the allocator's granularity, would not show here).
The per-slot scratch (split-K partial sums, the fused pose head's tile sums) is freed and reallocated when a larger batch follows
a smaller one: the results of the larger batch, and of the smaller one run again, must not depend on that."""
import numpy as np
import pytest

from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION

from helpers import hip_free_bytes
from test_pad_classes_gpu import sorted_layers

pytestmark = pytest.mark.gpu

H, W, B = 128, 416, 9


@pytest.fixture(scope="module")
def case():
    cfg = parse_version(FLAGSHIP_VERSION)
    return cfg, synth.make_inputs(B, H, W, first_window=11), synth.make_weights(cfg)


def _first(inputs, n):
    return tuple(np.ascontiguousarray(a[:n]) for a in inputs)


def _one_lifetime(cfg, inputs, weights):
    e = Engine(cfg, H, W, B)
    e.load_weights(weights)
    # the host staging group, the pad tables, the float32 tile orders, the fused pose head's tile scratch
    e.set_precision("f32")
    e.set_option("pad_classes", 15)
    e.forward(*inputs)
    # the split-K scratch
    e.set_precision("f16x3")
    e.forward(*_first(inputs, 1))
    assert e.last_split(4) > 1
    # the range ring: the records' mirrors, then the input snapshots
    two = _first(inputs, 2)
    bufs = [e.alloc(a.nbytes).upload(a) for a in two] + [e.alloc(2 * 12 * 4)]
    e.forward_device(2, *bufs)
    e.synchronize()
    for b in bufs:
        b.free()
    # the slots, the pose ring and the slots' staging sets
    e.set_inflight(4)
    one = _first(inputs, 1)
    outs = [np.empty((1, 2, 6), np.float32) for _ in range(4)]
    for out in outs:
        e.submit(*one, out)
    e.wait()
    e.set_inflight(1)
    # the event pool
    e.profile(1)
    e.forward(*one)
    assert e.profile_entries()
    # the feature export block
    e.set_feature_export(True)
    e.forward_features(*one)
    # every weight buffer a second time
    e.load_weights(weights)
    # the raw weight copies
    e.set_impl("direct")
    e.set_precision("f32")
    e.forward(*one)
    e.close()


def test_every_lazily_built_resource_goes_with_the_context(case):
    cfg, inputs, weights = case
    assert sorted_layers(H, W, B) == {"cnv4", "cnv5", "cnv6"}        # all three class-sorted tables are built, known not hoped for
    free = []
    for _ in range(3):                                               # the first lifetime also pays what the runtime keeps for the process
        _one_lifetime(cfg, inputs, weights)
        free.append(hip_free_bytes())
    assert free[1] == free[0] and free[2] == free[0], free


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_scratch_regrown_behind_a_smaller_batch_changes_no_bit(case, precision):
    cfg, inputs, weights = case
    one = _first(inputs, 1)

    def engine():
        e = Engine(cfg, H, W, B)
        e.load_weights(weights)
        e.set_precision(precision)
        return e

    a = engine()
    first = a.forward(*one)                  # the per-slot scratch is sized for one window ...
    grown = a.forward(*inputs)               # ... then freed and reallocated for nine
    again = a.forward(*one)
    a.close()
    b = engine()
    at_once = b.forward(*inputs)
    b.close()
    assert np.array_equal(grown, at_once)
    assert np.array_equal(again, first)

"""A live engine launches what tests/golden/forward_launches.json recorded, row by row: the launch count per profile label,
Engine.last_plan and Engine.last_split of one forward of every row of tests/forward_plan_cases.py (tests/test_forward_plan.py
derives the same table from davo_decide_forward on the CPU)."""
import json
import os

import pytest

import forward_plan_cases as FP

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_launches.json")
with open(GOLDEN) as f:
    RECORDED = {row["id"]: row for row in json.load(f)["rows"]}


@pytest.mark.parametrize("r", FP.ROWS, ids=FP.row_id)
def test_engine_launches_the_recorded_row(r):
    want = RECORDED[FP.row_id(r)]
    got = FP.observe(r)
    assert got["launches"] == want["launches"]
    assert got["last_plan"] == want["last_plan"]
    assert got["last_split"] == want["last_split"]

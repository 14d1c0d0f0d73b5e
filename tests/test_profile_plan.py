"""CPU: the summary-profile launch planner (netrep_amd/csrc/profile_plan.hip)
through its stand-alone check program, which build() makes beside the engine
library and which needs no GPU.

`carve` holds the LDS carve-outs of every kernel class against the byte
formulas the planner sizes them with. `plans` prints the plan of each shape of
a grid; tests/golden/profile_plans.json holds the same grid as the planner
planned it before it became one pure function (recorded once from that
commit's text, never regenerated from the code under test), so a launch
argument that moves shows here, without a GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "netrep_amd", "_lib", "profile_plan_check")
FIXTURE = os.path.join(ROOT, "tests", "golden", "profile_plans.json")

# the recorded planner's class integers
CLASS_NAME = {2: "packed", 4: "full_partials_in_scratch", 5: "small", 6: "full_vectors_in_scratch", 7: "wave"}

N_SAMPLES = [30, 112, 113, 200, 400, 1000, 1744, 2544, 2545, 2600]
K_MAX = [1, 111, 112, 113, 320, 321, 433, 434, 758, 759, 1733, 1734, 2554, 2555, 4200, 20000]
N_ITEMS = [1, 10**6]
# the data block's length decides between the wave and the small class only
# (32-bit byte offsets): none given, and one beyond them
DATA_DOUBLES = [0, 1 << 28]


def _run(*args, **kw):
    assert os.path.exists(CHECK), f"{CHECK} missing: __graft_entry__.build() makes it"
    return subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=120, **kw)


def test_carve_outs_match_byte_formulas():
    r = _run("carve")
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        d = json.load(f)
    assert "Never regenerate" in d["header"]
    rows = [dict(zip(d["fields"], r)) for r in d["rows"]]
    assert len(rows) == d["n_rows"]
    return d, rows


@pytest.fixture(scope="module")
def planned(recorded):
    d, rows = recorded
    assert d["cu"] == 256
    lines = "".join(f"{r['k_max']} {r['n_samples']} {r['n_items']} {r['data_doubles']}\n" for r in rows)
    r = _run("plans", input=lines)
    assert r.returncode == 0, r.stderr
    out = [dict(kv.split("=") for kv in ln.split()) for ln in r.stdout.splitlines()]
    table = [o for o in out if "table_kernel" in o]
    return [o for o in out if "table_kernel" not in o], table


def test_fixture_covers_the_grid(recorded):
    d, rows = recorded
    got = {(r["k_max"], r["n_samples"], r["n_items"], r["data_doubles"]) for r in rows}
    want = {(k, s, i, dd) for k in K_MAX for s in N_SAMPLES for i in N_ITEMS for dd in DATA_DOUBLES}
    assert got == want and len(rows) == len(want)
    # the recorded planner planned every class but the full Gram with its
    # partials in LDS ("variant 0"), which the enum no longer has
    assert d["variant0_rows"] == 0
    assert {r["class"] for r in rows} == set(CLASS_NAME)
    assert all(r["status"] == 0 for r in rows)


def test_plans_equal_the_recorded_planner(recorded, planned):
    _, rows = recorded
    plans, _ = planned
    assert len(plans) == len(rows)
    for exp, got in zip(rows, plans):
        exp = dict(exp)
        exp["class"] = CLASS_NAME[exp["class"]]
        assert set(got) == set(exp), (sorted(got), sorted(exp))
        for key, v in exp.items():
            assert got[key] == str(v), (key, got[key], v, exp)
        assert got["class"] in CLASS_NAME.values()


def test_table_rule_equals_the_recorded_one(recorded, planned):
    d, rows = recorded
    plans, table = planned
    n = 0
    for exp, got in zip(rows, plans):
        if exp["k_max"] <= 320:
            assert int(got["takes_table"]) == exp["takes_table"], exp
            n += exp["takes_table"]
    assert n > 0
    # and the launch it moves the segment to
    (t,) = table
    assert {"block": int(t["block"]), "lds": int(t["lds"])} == d["table_kernel"]

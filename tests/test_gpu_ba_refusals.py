"""Every refusal of the bundle adjustment's feature table (slam-tricks_amd/csrc/ba_features.hpp) through the C ABI, on
the a_chain case of ba_between_ref (tests/ba_refusal_cases.py).  tests/golden/ba_refusals.json holds the rows as the engine answered
when every function still carried its own checks.  Per row: an engine that holds the row's feature(s), the refused call, its return
code and stba_last_error() EQUAL to the golden text, the factor counts unchanged, and one iteration still solves.  Then: what the
golden file does not list is not refused (one held feature at a time), and the clearing call of every factor setter goes through on
an engine holding each feature its setting call conflicts with."""
import importlib
import json
import os

import pytest

import ba_refusal_cases as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_refusals.json")
with open(GOLDEN) as f:
    ROWS = json.load(f)["rows"]


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def row_id(r):
    return r["asker"].replace("stba_ba_", "") + "-" + "+".join(r["held"])


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_the_row_is_refused_with_its_text_and_the_engine_stays_usable(st, row):
    e = R.engine(st, row["held"])
    before = R.state(e)
    code, text = R.ask(st, e, R.SET[row["asker"]])
    assert code == row["code"]
    assert text == row["asker"] + ": " + row["text"]
    if row["asker"] in R.CLEAR:
        ccode, ctext = R.ask(st, e, R.CLEAR[row["asker"]])
        assert (ccode, ctext) == ((code, text) if row["when_clearing"] else (0, ""))
    if row["asker"] == "stba_ba_solve":           # (the one refusal made at solve time: without inner iterations the engine solves)
        e.set_inner_iterations(False)
    R.still_solves(st, e, before)


def test_what_the_table_does_not_list_is_not_refused(st):
    listed = {(r["asker"], tuple(r["held"])) for r in ROWS}
    for asker in R.SET:
        for f in R.FEATURES:
            if (asker, (f,)) not in listed:
                assert R.ask(st, R.engine(st, [f]), R.SET[asker]) == (0, ""), (asker, f)


def test_clearing_a_factor_is_never_refused(st):
    n = 0
    for asker in R.FACTOR_SETTERS:
        for r in (r for r in ROWS if r["asker"] == asker):
            for call in (R.CLEAR[asker], R.IDENTITY_WEIGHTS.get(asker)):
                if call is not None:
                    e = R.engine(st, r["held"])
                    before = R.state(e)
                    assert R.ask(st, e, call) == (0, ""), (asker, r["held"])
                    R.still_solves(st, e, before)
                    n += 1
    assert n == 19 + 6          # (every row of the five setters, and the all-identity weights on the six rows of the two weight setters)

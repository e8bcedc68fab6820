"""CPU suite: the generated translation unit and the refusal texts of every form of run-time-compiled objective are, byte
for byte, the ones recorded in tests/golden/objective_sources.json (tests/golden/make_objective_sources_golden.py: what is
recorded and how).  The same text with the same flags gives the same code object, so a change to how the text is put together
that passes here changes no kernel."""
import json
import os

import pytest

from golden import make_objective_sources_golden as M


@pytest.fixture(scope="module")
def now():
    return M.collect()


@pytest.fixture(scope="module")
def golden():
    with open(M.OUT) as f:
        return json.load(f)


def test_the_golden_covers_every_form_dtype_K_D_and_second_body(golden):
    forms = ("term", "chain", "grid", "graph", "mesh", "linear")
    per_dtype = {"term": 2, "chain": 2, "grid": 1, "graph": 3, "mesh": 27, "linear": 3}  # accepted K (x D) x second body
    for form in forms:
        for dname in ("f64", "f32"):
            assert sum(k.startswith("%s/%s/" % (form, dname)) for k in golden["sources"]) == per_dtype[form], (form, dname)
        for case in ("dtype=7", "body=null", "body=empty", "body=" + M.WORD):
            assert form + "/" + case in golden["refusals"]
    assert len(golden["sources"]) == 2 * sum(per_dtype.values())
    assert sorted(golden["bind"]) == ["graph", "grid", "linear", "mesh"]


@pytest.mark.parametrize("part", ["sources", "refusals", "bind"])
def test_generated_sources_and_refusals_are_the_recorded_bytes(now, golden, part):
    assert sorted(now[part]) == sorted(golden[part])
    for key, text in golden[part].items():
        assert now[part][key].encode() == text.encode(), key

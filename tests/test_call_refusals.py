"""Which pipeline calls are refused (no GPU): every case of tests/golden/call_refusals.json -- each switch of
tests/golden/make_call_refusals.py alone, every pair, and the hand-made cases -- replayed through the generator's
harness against the pipeline as it stands.  The fixture was written before the refusals were gathered into
stablediffusion_amd/combos.py, so the table answers to the checks it replaced and not to itself."""
import importlib.util
import itertools
import json
import os
import re

import pytest

from stablediffusion_amd import combos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_call_refusals",
                                               os.path.join(ROOT, "tests", "golden", "make_call_refusals.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.OUT) as _f:
    FIXTURE = json.load(_f)


@pytest.fixture(scope="module")
def replay():
    """{case id: (outcome, untouched, the row of REFUSALS that fired or None)}: every case runs once."""
    fired = []
    matching = combos.matching

    def spy(facts):
        fired.append(matching(facts))
        return fired[-1]
    combos.matching = spy
    try:
        out = {}
        for cid, names, extra, cfg_on in gen.cases():
            del fired[:]
            outcome, untouched = gen.run(names, cfg_on, extra)
            out[cid] = (outcome, untouched, next((r for r in fired if r is not None), None))
    finally:
        combos.matching = matching
    return out


def test_the_fixture_holds_every_case_and_every_pair():
    ids = [c[0] for c in FIXTURE["cases"]]
    assert ids == [c[0] for c in gen.cases()] and len(set(ids)) == len(ids)
    assert FIXTURE["untouched"] == list(gen.UNTOUCHED)
    paired = [n for n in gen.SWITCHES if n not in gen.HAND_ONLY]
    assert len(paired) == 29
    left_out = {frozenset(p[:2]) for p in FIXTURE["unbuildable"]}
    assert left_out == {frozenset(p) for p in gen.UNBUILDABLE} and len(left_out) == 5
    for n in paired:
        assert n in ids and n + "/no_cfg" in ids
    for a, b in itertools.combinations(paired, 2):
        assert (a + "+" + b in ids) != (frozenset((a, b)) in left_out), (a, b)


def test_every_case_ends_as_the_fixture_says(replay):
    wrong = []
    for case in FIXTURE["cases"]:
        cid, want = case[0], case[1]
        outcome, untouched, _ = replay[cid]
        if outcome != want:
            wrong.append((cid, want, outcome))
        elif len(case) == 3:             # refused: nothing that was untouched then is touched now
            wrong += [(cid, "touched", k) for k, v in case[2].items() if v and not untouched[k]]
    assert not wrong, wrong[:10]


def test_a_refusal_of_the_table_touches_nothing(replay):
    for cid, (outcome, untouched, row) in replay.items():
        if row is not None:
            assert outcome[0] == row.exc.__name__ and all(untouched.values()), (cid, outcome, untouched)


def test_every_row_fires_and_no_other_refusal_is_a_combination(replay):
    rows = {id(row) for _, _, row in replay.values() if row is not None}
    dead = [row.message for row in combos.REFUSALS if id(row) not in rows]
    assert not dead, dead
    assert len(combos.REFUSALS) == len({(r.when, r.message) for r in combos.REFUSALS})
    # a case the table refused reports that row; a case it let pass reports none of the table's messages but the one
    # encode_prompt shares with it
    shared = "the refiner reads text_encoder_2 / tokenizer_2, which this model does not have"
    messages = {r.message for r in combos.REFUSALS} - {shared}
    for cid, (outcome, _, row) in replay.items():
        if row is None:
            assert len(outcome) == 1 or outcome[1] not in messages, cid


def test_call_facts_is_the_only_reader():
    """Outside combos.py nothing decides a refusal: the facts' definitions stand in call_facts alone."""
    src = {n: open(os.path.join(ROOT, "stablediffusion_amd", n)).read() for n in ("pipeline.py", "regions.py", "combos.py")}
    pipeline, regions = src["pipeline.py"], src["regions.py"]
    assert pipeline.count("has_controlnet") == 1 and "def has_controlnet(self)" in pipeline       # the property itself
    assert "has_controlnet" not in regions
    for text in (pipeline, regions):
        assert not re.search(r"""["']time_cond_proj_dim["']""", text)          # (prose mentions it; no getattr does)
        assert not re.search(r"config\.time_cond_proj_dim", text)
        assert "float(pag_scale) > 0.0" not in text and "locals())" not in text
    assert src["combos.py"].count('"has_controlnet"') == 1 and src["combos.py"].count('"time_cond_proj_dim"') == 1
    assert pipeline.count("_combos.refuse(") == 1 and pipeline.count("_combos.call_facts(") == 1
    for gone in ("_check_pix2pix", "does not address the refiner", "(unload_controlnet)", "(disable_tome)",
                 "(disable_deepcache)"):
        assert gone not in pipeline and gone not in regions, gone


def test_the_documented_matrix_is_the_tables():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert combos.render_matrix() in doc
    names = [n for n, _ in combos.FEATURES]
    assert len(set(names)) == len(names)
    listed = {f.lstrip("!") for _, facts in combos.FEATURES for f in facts}
    assert listed <= set(combos.FACTS) and set(combos.FACTS) < set(combos.CallFacts._fields)

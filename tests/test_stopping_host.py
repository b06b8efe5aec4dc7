"""CPU: how a generation ends (`aurora_amd.stopping`).
  1. the definition against transformers' StopStringCriteria / EosTokenCriteria on the tiny tokenizer, exactly;
  2. the byte table against `clean_tokenizer_vocab`, and the byte-fallback rule;
  3. each known wrong implementation differs from the definition on some case of the suite;
  4. `check_stop`, the order of the four reasons, `finish_reason`, the record layout;
  5. the wiring: engine.caption_stream with a recording fake, llm.generate, the model's caption calls, the adaptor, the CLI."""
import ctypes
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from aurora_amd import _lib
from aurora_amd import stopping as ST
from tests import stopping_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 17


@pytest.fixture(scope="module")
def tiny():
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(SC.TINY)
    return tok, ST.token_bytes(tok)


# --------------------------------------------------------------------------------------------------- 1. against transformers
def test_the_definition_is_transformers_criteria_on_the_tiny_tokenizer(tiny):
    from transformers.generation.stopping_criteria import EosTokenCriteria, StopStringCriteria
    tok, table = tiny
    crit, eos = StopStringCriteria(tok, SC.STRINGS), EosTokenCriteria(EOS)
    assert crit._stop_string_matching_mode is None
    rec = ST.check_stop(dict(strings=SC.STRINGS), None, table)
    seqs = SC.seeded_sequences()
    assert len(seqs) == 3000 and all(1 <= len(h) <= 12 and 3 <= min(h) and max(h) < 300 for h in seqs)
    fired = by_eos = 0
    for h in seqs:
        ids = torch.tensor([h])
        s, e = bool(crit(ids, None)[0]), bool(eos(ids, None)[0])
        got = ST.fires(h, rec, table, None, 64)
        assert (got is not None) == s and (got is None or got[0] == "stop_string"), (h, got, s)
        got = ST.fires(h, rec, table, EOS, 64)
        assert (got is not None) == (s or e) and (not e or got == ("eos", None)), (h, got, s, e)
        fired += s
        by_eos += e
    assert 100 <= fired <= 2900 and fired == 262 and by_eos >= 3              # neither answer passes by default


def test_the_docstring_examples_of_stop_string_criteria():
    table, _ = SC.doc_table()
    rec = ST.check_stop(dict(strings="stop"), None, table)
    cases = SC.doc_cases()
    assert len(cases) == 9 and sum(f for _, f in cases) == 6
    for h, want in cases:
        assert (ST.fires(h, rec, table, None, 64) == ("stop_string", 0)) == want, h


# ---------------------------------------------------------------------------------------------------------- 2. the byte table
def test_token_bytes_is_clean_tokenizer_vocab_as_utf8(tiny):
    from transformers.generation.stopping_criteria import StopStringCriteria
    tok, table = tiny
    toks, idx = StopStringCriteria.clean_tokenizer_vocab(tok)
    assert len(idx) == 300 and len(table[0]) == 301 and table[0].dtype == np.int32 and table[1].dtype == np.uint8
    for s, i in zip(toks, idx):
        assert ST.bytes_of(table, i) == s.encode("utf-8"), i
    assert any(b" " in ST.bytes_of(table, i) for i in idx)                   # multi-word tokens
    assert ST.bytes_of(table, 300) is None and ST.bytes_of(table, -1) is None and ST.bytes_of(None, 3) is None
    wide = ST.token_bytes(tok, 320)                                          # ids the vocabulary does not name: inside the table, no bytes
    assert len(wide[0]) == 321 and ST.bytes_of(wide, 310) == b"" and ST.bytes_of(wide, 5) == ST.bytes_of(table, 5)


def test_byte_fallback_tokens_are_single_bytes():
    assert ST.token_text_bytes("<0x0A>", "<0x0A>") == b"\n" and ST.token_text_bytes("<0xe2>", "�") == b"\xe2"
    assert ST.token_text_bytes("<0xFF>", "") == b"\xff"
    for plain in ("<0x0G>", "<0x0A>>", "x<0x0A>", "<0x0a", "0x0A"):
        assert ST.token_text_bytes(plain, plain) == plain.encode()
    assert ST.token_text_bytes("▁the", " the") == b" the" and ST.token_text_bytes("é", "é") == "é".encode("utf-8")
    with pytest.raises(ValueError):
        ST.table_from_list([b"a", b"x" * 256])
    assert len(ST.table_from_list([b"x" * 255])[1]) == 255


# -------------------------------------------------------------------------------------------------------------------- 3. mutants
def variant_fires(kind, h, rec, table, eos, bmax):
    """`stopping.fires` written out again, with one known mistake switched on by `kind` (None: none)"""
    n, t = len(h), int(h[-1])
    rec = rec or {}
    if eos is not None and t == eos:
        return "eos", None
    ids = list(rec.get("token_ids", ()))
    probe = int(h[-2]) if kind == "id_on_previous_token" and n >= 2 else t
    if probe in ids:
        return "stop_token", ids.index(probe)
    tb = ST.bytes_of(table, t)
    if tb:
        window = 62 if kind == "window_62" else 63
        front = b""
        for x in reversed(list(h[:-1])):
            if len(front) >= window:
                break
            xb = ST.bytes_of(table, int(x))
            if xb is None:
                break
            front = xb + front
        front = front[-window:] if front else front
        text = front + tb
        strings = list(rec.get("strings", ()))
        for i, s in enumerate(strings[:1] if kind == "first_string_only" else strings):
            lo = len(front) if kind in ("end_at_the_boundary", "ends_before_t") else len(front) + 1
            if kind == "ends_before_t":
                lo = len(s)
            ends = [len(text)] if kind == "no_right_overhang" else range(lo, len(text) + 1)
            for end in ends:
                start = end - len(s)
                if kind == "no_left_overhang" and start < len(front):
                    continue
                if s and start >= 0 and text[start:end] == s:
                    return "stop_string", i
    budget = int(rec.get("max_new_tokens", 0) or 0)
    if kind == "budget_late":
        budget += 1 if budget else 0
    if kind == "budget_early":
        budget -= 1 if budget > 1 else 0
    if n >= bmax or (budget > 0 and n >= budget):
        return "length", None
    return None


def all_cases(tiny):
    """(history, record dict, table, eos, batch_max_new): the seeded sequences, the docstring examples and the edges"""
    _, table = tiny
    rec = ST.check_stop(dict(strings=SC.STRINGS), None, table)
    out = [(h, rec, table, None, 64) for h in SC.seeded_sequences()]
    dt, _ = SC.doc_table()
    out += [(h, ST.check_stop(dict(strings="stop"), None, dt), dt, None, 64) for h, _ in SC.doc_cases()]
    out += [(h, ST.from_record(r), SC.edge_table(), None, bmax) for h, r, bmax, _ in SC.edge_rows() if h]
    return out


MUTANTS = ["no_right_overhang", "no_left_overhang", "ends_before_t", "end_at_the_boundary", "window_62", "first_string_only", "budget_late",
           "budget_early", "id_on_previous_token"]


@pytest.mark.parametrize("kind", MUTANTS)
def test_each_known_mistake_differs_from_the_definition_on_some_case(tiny, kind):
    assert any(variant_fires(kind, *c) != ST.fires(*c) for c in all_cases(tiny)), kind


def test_the_variant_scaffold_without_a_mistake_is_the_definition(tiny):
    assert all(variant_fires(None, *c) == ST.fires(*c) for c in all_cases(tiny))


# ------------------------------------------------------------------------------------------------- 4. arguments, order, records
def test_check_stop_ranges():
    tab = SC.edge_table()
    assert ST.check_stop(None) is None and ST.check_stop({}) is None
    assert ST.check_stop(dict(token_ids=[], strings=[], max_new_tokens=0)) is None
    assert ST.check_stop(dict(token_ids=None, strings=None, max_new_tokens=None)) is None
    assert ST.check_stop(dict(max_new_tokens=24), 24) is None                # the batch's own limit asks nothing
    assert ST.check_stop(dict(max_new_tokens=24)) == dict(token_ids=(), strings=(), max_new_tokens=24)
    assert ST.check_stop(dict(strings="ab", token_ids=[np.int64(3), 5]), 24, tab) == dict(token_ids=(3, 5), strings=(b"ab",), max_new_tokens=0)
    assert ST.check_stop(dict(strings=["é", b"\xff"]), None, tab)["strings"] == ("é".encode(), b"\xff")
    assert ST.check_stop(dict(strings=["x" * 64], token_ids=list(range(8))), None, tab) is not None
    assert ST.check_stop(dict(strings=["ab"]), need_table=False) is not None
    for bad in (dict(strings=["ab"]),                                        # no byte table
                dict(unknown=1), "ab", [dict()]):
        with pytest.raises(ValueError):
            ST.check_stop(bad)
    for bad in (dict(strings=[""]), dict(strings=["x" * 65]), dict(strings=["é" * 33]), dict(strings=["a"] * 9), dict(strings=[3]),
                dict(token_ids=list(range(9))), dict(token_ids=[-1]), dict(token_ids=[2 ** 31]), dict(token_ids=[1.5]), dict(token_ids=[True]),
                dict(max_new_tokens=-1), dict(max_new_tokens=25), dict(max_new_tokens=2.0), dict(max_new_tokens=True)):
        with pytest.raises(ValueError):
            ST.check_stop(bad, 24, tab)
    assert ST.per_sequence(None, 3) is None and ST.per_sequence(dict(max_new_tokens=0), 3) is None and ST.per_sequence([None, {}], 2) is None
    one = ST.per_sequence(dict(token_ids=[4]), 3, 24)
    assert len(one) == 3 and one[0] == one[2] == dict(token_ids=(4,), strings=(), max_new_tokens=0)
    assert ST.per_sequence([None, dict(max_new_tokens=2)], 2, 24) == [None, dict(token_ids=(), strings=(), max_new_tokens=2)]
    with pytest.raises(ValueError):
        ST.per_sequence([None], 2)


def test_the_order_of_the_four_reasons_and_finish_reason():
    tab = SC.edge_table()
    A, B, AB = 0, 1, 3
    rec = ST.check_stop(dict(token_ids=[7, AB], strings=["x", "ab"], max_new_tokens=2), None, tab)
    h = [A, AB]                                                               # all four hold: EOS, stop id, "ab", budget 2
    assert ST.fires(h, rec, tab, AB, 64) == ("eos", None)
    assert ST.fires(h, rec, tab, None, 64) == ("stop_token", 1) == ST.fires(h, rec, tab, -1, 64)
    assert ST.fires(h, dict(rec, token_ids=()), tab, None, 64) == ("stop_string", 1)
    assert ST.fires(h, dict(rec, token_ids=(), strings=(b"ab", b"b")), tab, None, 64) == ("stop_string", 0)      # the lowest index
    assert ST.fires(h, dict(rec, token_ids=(), strings=()), tab, None, 64) == ("length", None)
    assert ST.fires(h, None, tab, None, 2) == ("length", None) and ST.fires(h, None, tab, None, 3) is None
    assert ST.fires([A, B], dict(strings=(b"ab",)), None, None, 64) is None  # no table: no bytes
    for eos, want in ((AB, ("eos", None)), (None, ("stop_token", 1))):
        assert ST.finish_reason(h, rec, tab, eos, 64) == want
    assert ST.finish_reason([A], rec, tab, None, 64) == (None, None) == ST.finish_reason([], rec, tab, None, 64)
    free = [A, A, B, A, AB, A]
    assert ST.first_stop(free, dict(strings=(b"ab",)), tab, None, 64) == 3 and ST.first_stop(free, dict(token_ids=(AB,)), tab, None, 64) == 5
    assert ST.first_stop(free, dict(max_new_tokens=4), tab, None, 64) == 4 and ST.first_stop(free, None, tab, None, 64) is None
    assert ST.first_stop(free, None, tab, B, 64) == 3


def test_record_layout_matches_the_c_struct_and_the_abi_lists_the_entry_points():
    src = open(os.path.join(ROOT, "include", "aurora_hip.h")).read()
    fields = _lib.AurStopRules._fields_
    assert ST.RECORD.itemsize == 592 == ctypes.sizeof(_lib.AurStopRules) and ST.RECORD.itemsize % 8 == 0
    assert list(ST.RECORD.names) == [n for n, _ in fields]
    assert [ST.RECORD.fields[n][1] for n in ST.RECORD.names] == [getattr(_lib.AurStopRules, n).offset for n, _ in fields]
    body = src[src.index("typedef struct aur_stop_rules {"):src.index("} aur_stop_rules;")]
    assert [m for m in re.findall(r"\b(max_new_tokens|n_token_ids|n_strings|reserved|token_ids|string_len|strings)\b[,;\[]", body)] == \
        ["max_new_tokens", "n_token_ids", "n_strings", "reserved", "token_ids", "string_len", "strings"]
    for name, val in (("AUR_STOP_MAX_IDS", ST.MAX_IDS), ("AUR_STOP_MAX_STRINGS", ST.MAX_STRINGS), ("AUR_STOP_MAX_STRING_BYTES", ST.MAX_STRING_BYTES),
                      ("AUR_STOP_MAX_TOKEN_BYTES", ST.MAX_TOKEN_BYTES)):
        assert re.search(rf"#define {name} {val}\b", src)
    r = ST.records([None, dict(token_ids=(5, 9), strings=(b"ab", b"xyz"), max_new_tokens=7)])
    assert not r[0:1].tobytes().strip(b"\0")                                 # neutral = all zero
    c = _lib.AurStopRules.from_buffer_copy(r[1:2].tobytes())
    assert (c.max_new_tokens, c.n_token_ids, c.n_strings, c.reserved) == (7, 2, 2, 0) and list(c.token_ids)[:3] == [5, 9, 0]
    assert list(c.string_len)[:3] == [2, 3, 0] and bytes(c.strings[1])[:4] == b"xyz\0"
    assert ST.from_record(r[1]) == dict(token_ids=(5, 9), strings=(b"ab", b"xyz"), max_new_tokens=7)
    for name in ("aur_slot_stop", "aur_stop_vocab", "aur_stop_rows"):
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", src)
    assert "stop.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES


# ---------------------------------------------------------------------------------------------------------------------- 5. the wiring
class _RecordingEngine:
    """enough of AuroraCapEngine for its own `caption_stream` (overlap=False) to run on the host: every call is logged in order"""
    max_batch, spare_slots, prefix_cache, _stop_table = 2, 0, 0, SC.edge_table()

    def __init__(self, lengths):
        self.log, self.lengths, self.owner, self.steps, self._stop_mode = [], lengths, {}, {}, False

    def _stop_on(self):
        self.log.append(("stop_on",))
        self._stop_mode = True

    def begin_batch(self, B, n, eos):
        self.log.append(("begin", B, n, eos))

    def slot_retire(self, s):
        pass

    def tome_r(self, *a):
        return 0

    def vit_encode(self, px, r):
        return px

    def project_splice(self, vis, ids, plan=None):
        return ids, len(ids)

    def slot_reset(self, s):
        self.log.append(("reset", s))

    def slot_stop(self, s, recs):
        self.log.append(("stop", s, ST.from_record(recs[0])))

    def prefill(self, s, emb, L):
        self.log.append(("prefill", s, emb[0]))
        self.owner[s], self.steps[s] = emb[0], 1

    def decode(self, n):
        for s in self.steps:
            self.steps[s] += n

    def slot_state(self):
        fin = [int(s in self.owner and self.steps[s] >= self.lengths[self.owner[s]]) for s in range(2)]
        return [0, 0], fin

    def outputs(self, lpn):
        return {s: [self.owner[s]] for s in self.owner}


def run_stream(eng, n_clips, **kw):
    from aurora_amd.engine import AuroraCapEngine
    clips = [(torch.zeros(1, 3, 4, 4), [i]) for i in range(n_clips)]
    return dict(AuroraCapEngine.caption_stream(eng, clips, 0.5, 8, eos_id=None, slots=2, check_every=1, overlap=False, **kw))


def test_caption_stream_gives_each_refilled_slot_its_clips_record_before_its_prefill():
    stops = [dict(token_ids=[3]), None, dict(max_new_tokens=2), dict(strings=["ab"]), dict(max_new_tokens=8)]
    e = _RecordingEngine([3, 1, 2, 1, 1])
    asked = []

    def stop_of(i):
        asked.append(i)
        return stops[i]
    assert run_stream(e, 5, stop=stop_of) == {i: [i] for i in range(5)}
    assert e.log[0] == ("stop_on",) and e.log[1][0] == "begin" and asked == list(range(5))
    fills = [(e.log[k - 2], e.log[k - 1], e.log[k]) for k in range(len(e.log)) if e.log[k][0] == "prefill"]
    assert len(fills) == 5
    neutral = dict(token_ids=(), strings=(), max_new_tokens=0)
    for a, b, c in fills:                                                    # reset, then the record, then the prefill - on one slot
        i = c[2]
        want = ST.check_stop(stops[i], 8, SC.edge_table()) or neutral        # a budget equal to the batch's is neutral
        assert a == ("reset", c[1]) and b == ("stop", c[1], want), (a, b, c)
    assert {c[1] for _, _, c in fills} == {0, 1} and [c[1] for _, _, c in fills][:2] == [0, 1]      # both slots, re-used
    # one dict for every clip; None and a neutral dict: the path of a call without the argument
    e = _RecordingEngine([1, 2, 1])
    run_stream(e, 3, stop=dict(token_ids=[4]))
    assert [x for x in e.log if x[0] == "stop"] == [("stop", s, dict(token_ids=(4,), strings=(), max_new_tokens=0)) for s in (0, 1, 0)]
    for unasked in (None, dict(token_ids=[], max_new_tokens=0), dict(max_new_tokens=8)):
        e = _RecordingEngine([1, 2, 1])
        run_stream(e, 3, stop=unasked)
        assert not e._stop_mode and not [x for x in e.log if x[0] in ("stop", "stop_on")]
    # a record the host rejects is that clip's own error
    e, errs = _RecordingEngine([1, 1, 1]), []
    got = run_stream(e, 3, stop=lambda i: dict(strings=["x" * 65]) if i == 1 else None, on_error=lambda i, ex: errs.append((i, type(ex))))
    assert got == {0: [0], 2: [2]} and errs == [(1, ValueError)]
    with pytest.raises(ValueError):
        run_stream(_RecordingEngine([1]), 1, stop=dict(max_new_tokens=9))    # more than the batch's limit


class _FakeEngine:
    dev, max_new_tokens, l, v, max_batch = "cpu", 64, {"hidden_size": 8, "vocab_size": 320}, {}, 4

    def __init__(self):
        self.calls, self.tables = [], []

    def set_stop_vocab(self, table):
        self.tables.append(table)

    def generate(self, embeds, lens, n, eos_id=2, **kw):
        self.calls.append(dict(kw, eos_id=eos_id))
        return [[1, 2, 3]]

    def caption_batch(self, clips, ratio, n, eos, **kw):
        self.calls.append(kw)
        return [[1] for _ in clips]

    def caption_stream(self, clips, ratio, n, eos, **kw):
        self.calls.append({k: v for k, v in kw.items() if v is not None})
        for k, _ in enumerate(clips):
            yield k, [1]


def test_llm_generate_keyword_mapping(tiny):
    from aurora_amd.model import _LLM, split_stop_arguments
    tok, table = tiny
    e = _FakeEngine()
    llm = _LLM(e, 2)
    x = torch.zeros(1, 5, 8)
    llm.generate(inputs_embeds=x)
    assert e.calls[-1] == dict(eos_id=2) and not e.tables
    llm.generate(inputs_embeds=x, stop_strings=["the door", "."], tokenizer=tok)
    assert e.calls[-1] == dict(eos_id=2, stop=dict(token_ids=[], strings=["the door", "."]))
    assert len(e.tables) == 1 and np.array_equal(e.tables[0][1][:len(table[1])], table[1]) and len(e.tables[0][0]) == 321
    llm.generate(inputs_embeds=x, stop_strings="ss", tokenizer=tok)          # one string; the table is built once per tokenizer
    assert e.calls[-1]["stop"] == dict(token_ids=[], strings=["ss"]) and len(e.tables) == 1
    llm.generate(inputs_embeds=x, eos_token_id=[2, 5, 9])                    # the first id is the EOS, the rest are stop ids
    assert e.calls[-1] == dict(eos_id=2, stop=dict(token_ids=[5, 9], strings=[])) and len(e.tables) == 1
    llm.generate(inputs_embeds=x, eos_token_id=[7], stop_token_ids=[7, 4, 4])
    assert e.calls[-1] == dict(eos_id=7, stop=dict(token_ids=[4], strings=[]))
    llm.generate(inputs_embeds=x, eos_token_id=None, stop_token_ids=[])
    assert e.calls[-1] == dict(eos_id=None)
    n = len(e.calls)
    with pytest.raises(ValueError):
        llm.generate(inputs_embeds=x, stop_strings=["ss"])                   # transformers requires the tokenizer too
    assert len(e.calls) == n
    assert split_stop_arguments([], None, None) == (None, None) and split_stop_arguments(3, "a", [3]) == (3, dict(token_ids=[], strings=["a"]))


def test_model_caption_calls_pass_stop_down():
    from aurora_amd.model import AuroraModel
    e = _FakeEngine()
    m = AuroraModel(e, eos_token_id=2)
    clip = (torch.zeros(1, 3, 4, 4), [1, -200, 5])
    stop = dict(token_ids=[4])
    m.caption_batch([clip], max_new_tokens=8)
    assert "stop" not in e.calls[-1]
    m.caption_batch([clip] * 6, max_new_tokens=8, stop=stop)
    assert e.calls[-1]["stop"] == stop and e.calls[-2]["stop"] == stop       # two chunks of max_batch 4
    per = [None, stop, None, None, dict(max_new_tokens=2), None]
    m.caption_batch([clip] * 6, max_new_tokens=8, stop=per)
    assert e.calls[-2]["stop"] == per[:4] and e.calls[-1]["stop"] == per[4:]
    with pytest.raises(ValueError):
        m.caption_batch([clip] * 2, max_new_tokens=8, stop=[stop])
    m.caption_prompts(clip[0], [clip[1], clip[1]], max_new_tokens=8, stop=[stop, None])
    assert e.calls[-1]["stop"] == [stop, None] and e.calls[-1]["share"] == [0, 0]
    f = lambda i: stop                                                       # noqa: E731
    assert dict(m.caption_stream([clip], max_new_tokens=8, stop=f)) == {0: [1]} and e.calls[-1]["stop"] is f
    assert dict(m.caption_stream([clip], max_new_tokens=8)) == {0: [1]} and "stop" not in e.calls[-1]


def test_plugin_honor_until_off_and_on():
    from tests.test_sampling_host import _BatchModel, _StreamModel, _plugin, _requests
    from tests.test_lmms_plugin import FakeTok
    P, _ = _plugin(_BatchModel())
    assert P.gen_stop({}) == (None, []) and P.gen_stop({"until": ["\n"]}) == (None, [])                      # off: dropped as before
    assert P.gen_stop({"until": ["\n", "", "</s>", "\n"]}, True, "</s>") == (dict(token_ids=(), strings=(b"\n",), max_new_tokens=0), ["\n"])
    assert P.gen_stop({"until": "Q:"}, True) == (dict(token_ids=(), strings=(b"Q:",), max_new_tokens=0), ["Q:"])
    assert P.gen_stop({"until": ["</s>"]}, True, "</s>") == (None, [])
    assert P.gen_stop({"stop_token_ids": [5, 6]}) == (dict(token_ids=(5, 6), strings=(), max_new_tokens=0), [])
    for bad, on in (({"until": ["x" * 65]}, True), ({"until": [str(i) for i in range(9)]}, True), ({"until": [3]}, True), ({"until": 3}, True),
                    ({"stop_token_ids": "5"}, False), ({"stop_token_ids": [1.5]}, False), ({"stop_token_ids": list(range(9))}, False)):
        with pytest.raises(ValueError):
            P.gen_stop(bad, on)
    assert P.gen_defaults({"until": ["\n"], "stop_token_ids": [5]}) == {"max_new_tokens": 1024, "temperature": 0, "top_p": None, "num_beams": 1}
    text = FakeTok().batch_decode([[7]], skip_special_tokens=True)[0]
    until = {"until": [text[:1] if len(text) > 1 else "zz", "Q:"]}
    docs, reqs = _requests([until, {}, {"stop_token_ids": [9]}, until])
    for on in (False, True):
        for model in (_BatchModel(), _StreamModel()):
            used = []
            model.llm = SimpleNamespace(use_tokenizer=used.append)
            P, m = _plugin(model, honor_until=on)
            m.task_dict = {"t": {"s": docs}}
            res = m.generate_until(reqs)
            stops = [c[1].get("stop") for c in model.calls]
            with_ids = [s for s in stops if s and s["token_ids"]]
            with_str = [s for s in stops if s and s["strings"]]
            assert with_ids and all(s == dict(token_ids=(9,), strings=(), max_new_tokens=0) for s in with_ids)
            assert res[1] == res[2] == text
            if on:
                assert with_str and all(s["strings"] == tuple(t.encode() for t in until["until"]) for s in with_str) and len(used) >= 1
                assert res[0] == res[3] == text.split(until["until"][0])[0]
            else:
                assert not with_str and not used and res[0] == res[3] == text


def test_cli_arguments():
    import inference
    a = inference.build_parser().parse_args([])
    assert (a.stop, a.stop_token_id) == ([], [])
    a = inference.build_parser().parse_args(["--stop", "Q:", "--stop", "\n\n", "--stop_token_id", "5", "--stop_token_id", "9"])
    assert (a.stop, a.stop_token_id) == (["Q:", "\n\n"], [5, 9])
    for flags, word in ((["--stop", "x" * 65], "64"), (["--stop_token_id", "-1"], "token_ids"), (["--synthetic", "--stop", "ab"], "tokenizer")):
        bad = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py")] + flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and word in bad.stderr and "Traceback" not in bad.stderr, (flags, bad.stderr[-500:])

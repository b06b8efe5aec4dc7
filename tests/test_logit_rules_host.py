"""Logit rules, host side (no GPU): `aurora_amd.logit_rules.apply` against transformers' three processors bit for bit, against
deliberately wrong variants, and against transformers' own `generate(inputs_embeds=...)` on the checkpoint fixture (the history is the
generated tokens, not the prompt); the argument checks; and the wiring from `llm.generate` / the lmms-eval adaptor / the CLI down."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from aurora_amd import _lib
from aurora_amd import logit_rules as LR
from tests.logit_rules_cases import EOS, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- 1. the definition == transformers
def hf_apply(row, history, rules, eos_id):
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    ids = torch.tensor([list(history)], dtype=torch.long).reshape(1, len(history))
    s = torch.from_numpy(np.array(row, np.float32, copy=True)).unsqueeze(0)
    s = RepetitionPenaltyLogitsProcessor(penalty=rules["repetition_penalty"])(ids, s)
    if rules["no_repeat_ngram_size"] > 0:
        s = NoRepeatNGramLogitsProcessor(rules["no_repeat_ngram_size"])(ids, s)
    s = MinNewTokensLengthLogitsProcessor(prompt_length_to_skip=0, min_new_tokens=rules["min_new_tokens"], eos_token_id=eos_id)(ids, s)
    return s[0].numpy()


def test_the_definition_is_transformers_three_processors_bitwise():
    assert len(CASES) > 500
    seen = dict(pen=0, ban=0, eos=0)
    for tag, row, h, rules, eos in CASES:
        got, want = LR.apply(row, h, rules, eos), hf_apply(row, h, rules, eos)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), tag
        assert np.array_equal(bits(row), bits(LR.apply(row, h, None, eos)))                        # the input is never written
        changed = bits(got) != bits(row)
        seen["pen"] += int((changed & np.isfinite(got)).any())
        seen["ban"] += int(len(LR.banned_by_ngram(h, rules["no_repeat_ngram_size"])) > 0)
        seen["eos"] += int(len(h) < rules["min_new_tokens"])
    assert min(seen.values()) > 50, seen                                                           # every rule is really exercised
    # the order of the rules does not matter: the definition again with the bans ahead of the penalty
    for tag, row, h, rules, eos in CASES[::7]:
        banned = LR.apply(row, h, dict(rules, repetition_penalty=1.0), eos)
        swapped = LR.apply(banned, h, dict(repetition_penalty=rules["repetition_penalty"]), eos)
        assert np.array_equal(bits(swapped), bits(LR.apply(row, h, rules, eos))), tag


# --------------------------------------------------------------------------------------------- 2. the cases see the known mistakes
def _variant(kind):
    """`apply` with one deliberate mistake."""
    def f(row, h, rules, eos):
        l = np.array(row, np.float32, copy=True)
        n = len(h)
        p, g, m = np.float32(rules["repetition_penalty"]), rules["no_repeat_ngram_size"], rules["min_new_tokens"]
        with np.errstate(all="ignore"):
            if p != 1.0:
                if kind == "per_occurrence":
                    for t in h:
                        l[t] = l[t] * p if l[t] < 0 else l[t] / p
                else:
                    t = np.unique(np.asarray(h, np.int64))
                    o = l[t]
                    l[t] = o * p if kind == "mul_positive" else np.where(o < 0, o * p, o / p)
            banned = []
            if g > 0:
                if n + 1 >= g:
                    tail = h[n - g + 1:n]
                    rng = {"window_end": range(n - g), "window_start": range(1, n - g + 1)}.get(kind, range(n - g + 1))
                    banned = [h[i + g - 1] for i in rng if h[i:i + g - 1] == tail]
                elif kind == "short_history" and n > 0:                     # falls back to the longest n-gram that fits
                    banned = LR.banned_by_ngram(h, n)
            if eos is not None and (n <= m if kind == "eos_at_m" else n < m):
                banned = banned + [eos]
            for t in banned:
                l[t] = -np.abs(l[t]) * np.float32(np.inf) if kind == "zero_times_inf" else -np.inf
        return l
    return f


@pytest.mark.parametrize("kind", ["per_occurrence", "mul_positive", "window_end", "window_start", "short_history", "eos_at_m",
                                  "zero_times_inf"])
def test_each_known_mistake_differs_from_the_definition_on_some_case(kind):
    f = _variant(kind)
    differ = [tag for tag, row, h, rules, eos in CASES
              if not np.array_equal(bits(f(row, h, rules, eos)), bits(LR.apply(row, h, rules, eos)))]
    assert differ, kind
    print(kind, len(differ), "of", len(CASES), "cases, e.g.", differ[0])


def test_the_variant_scaffold_without_a_mistake_is_the_definition():
    f = _variant(None)
    assert all(np.array_equal(bits(f(row, h, rules, eos)), bits(LR.apply(row, h, rules, eos))) for _, row, h, rules, eos in CASES)


# ------------------------------------------------------------------------------- 3. the history is the generated tokens, not the prompt
def test_history_is_what_transformers_generate_sees_with_inputs_embeds():
    from transformers import LlamaForCausalLM
    model = LlamaForCausalLM.from_pretrained(os.path.join(ROOT, "tests", "golden", "ckpt_tiny"), torch_dtype=torch.float32).eval()
    emb = torch.randn(1, 10, model.config.hidden_size, generator=torch.Generator().manual_seed(0))
    N = 16
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = model.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=N, eos_token_id=None, pad_token_id=0)[0].tolist()
        eos = plain[2]                                                      # a token greedy emits early: min_new_tokens has work to do
        rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=6)
        want = model.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=N, eos_token_id=eos, pad_token_id=0, **rules)[0].tolist()
        stopped = model.generate(inputs_embeds=emb, do_sample=False, max_new_tokens=N, eos_token_id=eos, pad_token_id=0)[0].tolist()
        assert stopped == plain[:3] and len(want) >= 6 and want[:len(plain)] != plain[:len(want)]      # the rules change the output
        # the host loop: the same model's logits, `apply` over the generated tokens only
        got, past, x = [], None, emb
        while len(got) < N:
            out = model(inputs_embeds=x, past_key_values=past, use_cache=True)
            past = out.past_key_values
            row = LR.apply(out.logits[0, -1].float().numpy(), got, rules, eos)
            got.append(int(np.argmax(row)))
            if got[-1] == eos:
                break
            x = model.get_input_embeddings()(torch.tensor([[got[-1]]]))
    assert got == want, (got, want)


# ------------------------------------------------------------------------------------------------------- 4. argument checks, records
def test_check_logit_rules_ranges():
    assert LR.check_logit_rules(None) is None and LR.check_logit_rules({}) is None
    assert LR.check_logit_rules(dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)) is None
    assert LR.check_logit_rules(dict(repetition_penalty=None, no_repeat_ngram_size=None)) is None
    r = LR.check_logit_rules(dict(repetition_penalty=1.2))
    assert r == dict(repetition_penalty=float(np.float32(1.2)), no_repeat_ngram_size=0, min_new_tokens=0)
    assert LR.check_logit_rules(dict(no_repeat_ngram_size=3)) == dict(repetition_penalty=1.0, no_repeat_ngram_size=3, min_new_tokens=0)
    assert LR.check_logit_rules(dict(min_new_tokens=np.int64(4)))["min_new_tokens"] == 4
    assert LR.check_logit_rules(r) == r
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
                dict(repetition_penalty=float("inf")), dict(repetition_penalty="1.2"), dict(repetition_penalty=True),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True), dict(min_new_tokens=-3),
                dict(min_new_tokens="4"), dict(min_new_tokens=2 ** 31), dict(frequency_penalty=0.5)):
        with pytest.raises(ValueError):
            LR.check_logit_rules(bad)


def test_record_layout_matches_the_c_struct_and_the_abi_lists_the_entry_points():
    src = open(os.path.join(ROOT, "include", "aurora_hip.h")).read()
    fields = _lib.AurLogitRules._fields_
    assert LR.RECORD.itemsize == 16 == __import__("ctypes").sizeof(_lib.AurLogitRules)
    assert list(LR.RECORD.names) == [n for n, _ in fields]
    assert [LR.RECORD.fields[n][1] for n in LR.RECORD.names] == [getattr(_lib.AurLogitRules, n).offset for n, _ in fields]
    assert re.search(r"typedef struct aur_logit_rules \{ float repetition_penalty; int32_t no_repeat_ngram; int32_t min_new_tokens; "
                     r"int32_t reserved; \} aur_logit_rules;", src)
    r = LR.records(dict(repetition_penalty=1.25, no_repeat_ngram_size=3, min_new_tokens=9), 2)
    c = _lib.AurLogitRules.from_buffer_copy(r[1:2].tobytes())
    assert (c.repetition_penalty, c.no_repeat_ngram, c.min_new_tokens, c.reserved) == (1.25, 3, 9, 0)
    n = LR.records(None, 3)
    assert (n["repetition_penalty"] == 1.0).all() and not n["no_repeat_ngram"].any() and not n["min_new_tokens"].any()
    for name in ("aur_slot_logit_rules", "aur_logit_rules_rows"):
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", src)
    assert "logit_rules.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES


# ---------------------------------------------------------------------------------------------------------------------- 5. the wiring
class _FakeEngine:
    dev, max_new_tokens, l, v, max_batch = "cpu", 64, {"hidden_size": 8}, {}, 4

    def __init__(self):
        self.calls = []

    def generate(self, embeds, lens, n, eos_id=2, **kw):
        self.calls.append(kw)
        return [[1, 2, 3]]

    def caption_batch(self, clips, ratio, n, eos, **kw):
        self.calls.append(kw)
        return [[1] for _ in clips]

    def caption_stream(self, clips, ratio, n, eos, **kw):
        self.calls.append({k: v for k, v in kw.items() if v is not None})
        for k, _ in enumerate(clips):
            yield k, [1]


def test_llm_generate_passes_the_three_keywords_down():
    from aurora_amd.model import _LLM
    e = _FakeEngine()
    llm = _LLM(e, 2)
    x = torch.zeros(1, 5, 8)
    llm.generate(inputs_embeds=x)
    assert e.calls[-1] == {}
    llm.generate(inputs_embeds=x, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    assert e.calls[-1] == {}                                                 # neutral values: the path of a call that never asked
    llm.generate(inputs_embeds=x, repetition_penalty=1.25, no_repeat_ngram_size=3, min_new_tokens=7)
    assert e.calls[-1] == dict(logit_rules=dict(repetition_penalty=1.25, no_repeat_ngram_size=3, min_new_tokens=7))
    llm.generate(inputs_embeds=x, do_sample=True, temperature=0.5, no_repeat_ngram_size=2)
    assert e.calls[-1]["logit_rules"] == dict(repetition_penalty=1.0, no_repeat_ngram_size=2, min_new_tokens=0) and "sampling" in e.calls[-1]
    llm.generation_logit_rules = dict(repetition_penalty=1.5, min_new_tokens=4)      # the checkpoint's generation_config.json
    llm.generate(inputs_embeds=x)
    assert e.calls[-1] == dict(logit_rules=dict(repetition_penalty=1.5, no_repeat_ngram_size=0, min_new_tokens=4))
    llm.generate(inputs_embeds=x, repetition_penalty=1.0, min_new_tokens=0)          # an explicit argument wins
    assert e.calls[-1] == {}
    llm.generate(inputs_embeds=x, repetition_penalty=1.25)
    assert e.calls[-1] == dict(logit_rules=dict(repetition_penalty=1.25, no_repeat_ngram_size=0, min_new_tokens=4))
    n = len(e.calls)
    for bad in (dict(repetition_penalty=0.0), dict(no_repeat_ngram_size=-1), dict(min_new_tokens=-1), dict(repetition_penalty="x")):
        with pytest.raises(ValueError):
            llm.generate(inputs_embeds=x, **bad)
    assert len(e.calls) == n


def test_generation_config_values_are_read_from_the_checkpoint(tmp_path):
    from aurora_amd.model import generation_logit_rules
    assert generation_logit_rules(str(tmp_path)) == {}
    (tmp_path / "llm").mkdir()
    (tmp_path / "llm" / "generation_config.json").write_text('{"top_k": 40, "repetition_penalty": 1.1, "no_repeat_ngram_size": null}')
    assert generation_logit_rules(str(tmp_path)) == {"repetition_penalty": 1.1}
    assert generation_logit_rules(os.path.join(ROOT, "tests", "golden", "ckpt_tiny")) == {}


def test_model_caption_calls_pass_logit_rules_down():
    from aurora_amd.model import AuroraModel
    e = _FakeEngine()
    m = AuroraModel(e, eos_token_id=2)
    clip = (torch.zeros(1, 3, 4, 4), [1, -200, 5])
    rules = dict(no_repeat_ngram_size=3)
    full = dict(repetition_penalty=1.0, no_repeat_ngram_size=3, min_new_tokens=0)
    m.caption_batch([clip], max_new_tokens=8)
    assert "logit_rules" not in e.calls[-1]
    m.caption_batch([clip], max_new_tokens=8, logit_rules=dict(repetition_penalty=1.0))
    assert "logit_rules" not in e.calls[-1]
    m.caption_batch([clip], max_new_tokens=8, logit_rules=rules)
    assert e.calls[-1]["logit_rules"] == full
    m.caption_prompts(clip[0], [clip[1], clip[1]], max_new_tokens=8, logit_rules=rules)
    assert e.calls[-1]["logit_rules"] == full and e.calls[-1]["share"] == [0, 0]
    assert dict(m.caption_stream([clip], max_new_tokens=8, logit_rules=rules)) == {0: [1]}
    assert e.calls[-1]["logit_rules"] == full
    assert dict(m.caption_stream([clip], max_new_tokens=8)) == {0: [1]}
    assert "logit_rules" not in e.calls[-1]
    with pytest.raises(ValueError):
        m.caption_batch([clip], logit_rules=dict(repetition_penalty=-1))


def test_plugin_honours_the_three_gen_kwargs():
    from tests.test_sampling_host import _BatchModel, _StreamModel, _plugin, _requests
    P, _ = _plugin(_BatchModel())
    assert P.gen_logit_rules({}) is None and P.gen_logit_rules({"repetition_penalty": 1.0, "min_new_tokens": 0}) is None
    assert P.gen_logit_rules({"repetition_penalty": 1.5, "max_new_tokens": 8}) == dict(repetition_penalty=1.5, no_repeat_ngram_size=0, min_new_tokens=0)
    for bad in ({"repetition_penalty": "1.2"}, {"repetition_penalty": [1.2]}, {"no_repeat_ngram_size": 2.5}, {"min_new_tokens": "3"},
                {"no_repeat_ngram_size": -1}, {"repetition_penalty": 0}):
        with pytest.raises(ValueError):
            P.gen_defaults(bad)
    assert P.gen_defaults({"until": ["\n"]}) == {"max_new_tokens": 1024, "temperature": 0, "top_p": None, "num_beams": 1}
    ruled = {"no_repeat_ngram_size": 3, "repetition_penalty": 1.5, "min_new_tokens": 2}
    docs, reqs = _requests([ruled, {}, ruled, {}, ruled])
    for model in (_BatchModel(), _StreamModel()):
        P, m = _plugin(model)
        m.task_dict = {"t": {"s": docs}}
        assert m.generate_until(reqs) == ["7"] * 5
        with_rules = [c for c in model.calls if "logit_rules" in c[1]]
        without = [c for c in model.calls if "logit_rules" not in c[1]]
        assert with_rules and without
        assert all(c[1]["logit_rules"] == ruled for c in with_rules)
        count = (lambda c: c[0]) if isinstance(model, _BatchModel) and not isinstance(model, _StreamModel) else (lambda c: len(c[0]))
        assert sum(count(c) for c in with_rules) == 3 and sum(count(c) for c in without) == 2


def test_cli_flags():
    import subprocess
    import sys
    import inference
    a = inference.build_parser().parse_args([])
    assert (a.repetition_penalty, a.no_repeat_ngram_size, a.min_new_tokens) == (None, None, None)
    a = inference.build_parser().parse_args(["--repetition_penalty", "1.2", "--no_repeat_ngram_size", "3", "--min_new_tokens", "5"])
    assert (a.repetition_penalty, a.no_repeat_ngram_size, a.min_new_tokens) == (1.2, 3, 5)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--repetition_penalty", "0"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode != 0 and "repetition_penalty" in bad.stderr and "Traceback" not in bad.stderr


def test_eos_constant_is_a_history_token():
    assert any(EOS in h and len(h) < r["min_new_tokens"] for _, _, h, r, _ in CASES)

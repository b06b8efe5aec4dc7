"""Classifier-free guidance, host side (no GPU): `aurora_amd.guidance.apply` against transformers'
UnbatchedClassifierFreeGuidanceLogitsProcessor driven with a stub model, the argument checks, the slot pairing, the record layout and
the exports of the built library, and the wiring from `llm.generate` / `AuroraModel` / the lmms-eval adaptor / the CLI down."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from aurora_amd import _lib
from aurora_amd import guidance as GD
from tests import guidance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- 1. the definition == transformers
class _Out(dict):
    logits = property(lambda self: self["logits"])


class _Stub:
    """the `model` of the processor: whatever it is asked, the next-token logits are the given unconditional row"""
    def __init__(self, u):
        self.u, self.calls = u, 0

    def __call__(self, input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        self.calls += 1
        return _Out(logits=self.u.reshape(1, 1, -1).expand(1, input_ids.shape[1], -1))


def hf_apply(c, u, g, dtype):
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    stub = _Stub(torch.from_numpy(np.asarray(u)).to(dtype))
    proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(g, stub, unconditional_ids=torch.tensor([[1, 7]]), use_cache=False)
    out = proc(torch.tensor([[3]]), torch.from_numpy(np.asarray(c)).to(dtype).unsqueeze(0))
    assert stub.calls == 1
    return out[0].numpy()


def test_the_definition_is_transformers_processor():
    pairs = checked32 = 0
    for V, n in ((32000, 80), (1003, 180)):
        for k in range(n):
            rng = np.random.default_rng(100000 + 7 * V + k)
            c, u = R.row_pair(rng, V)
            for g in R.SCALES:
                want = GD.apply(c, u, g)
                got = hf_apply(c.astype(np.float64), u.astype(np.float64), g, torch.float64)
                assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12, (V, k, g)
                # float32, as transformers runs it: the same pick wherever the float64 margin exceeds the fp32 rounding of the row
                top = np.sort(want)[-2:]
                if top[1] - top[0] > 2 * R.bound(c, u, g):
                    assert int(np.argmax(hf_apply(c, u, g, torch.float32))) == int(np.argmax(want)), (V, k, g)
                    checked32 += 1
                pairs += 1
    assert pairs >= 1000 and checked32 > 0.95 * pairs, (pairs, checked32)


def test_guidance_moves_the_pick_away_from_the_prior():
    """what the feature is for: a token the negative prompt alone makes likely loses against one only the prompt supports"""
    V = 1003
    c = np.zeros(V, np.float32)
    u = np.zeros(V, np.float32)
    c[10], c[20] = 5.0, 4.5              # 10: the language prior's word (the negative prompt likes it as much); 20: what the frames show
    u[10] = 5.0
    assert int(np.argmax(c)) == 10
    assert int(np.argmax(GD.apply(c, u, 1.5))) == 20 and int(np.argmax(GD.apply(c, u, 0.5))) == 10


# ---------------------------------------------------------------------------------------------------------------- 2. the arguments
def test_scale_one_and_none_are_no_request():
    assert GD.check_guidance(None) is None
    assert GD.check_guidance(dict(scale=None)) is None
    assert GD.check_guidance(dict(scale=1)) is None and GD.check_guidance(dict(scale=1.0, negative_ids=[1, 2])) is None
    assert GD.check_scale(None) is None and GD.check_scale(1.0) is None and GD.check_scale(np.float32(1)) is None
    got = GD.check_guidance(dict(scale=2, negative_ids=[4, 5]))
    assert got == dict(scale=2.0, negative_ids=[4, 5])
    assert GD.check_guidance(dict(scale=0.1))["scale"] == float(np.float32(0.1))     # the value the kernel sees


@pytest.mark.parametrize("bad", [0, 0.0, -1, -2.5, float("inf"), float("-inf"), float("nan"), "2", True, 1e-50, 1e39])
def test_check_guidance_rejects_what_is_not_a_finite_positive_scale(bad):
    with pytest.raises(ValueError):
        GD.check_guidance(dict(scale=bad))
    with pytest.raises(ValueError):
        GD.check_scale(bad)


def test_check_guidance_rejects_unknown_keys_and_other_types():
    with pytest.raises(ValueError):
        GD.check_guidance(dict(scale=2, negativ=[1]))
    with pytest.raises(ValueError):
        GD.check_guidance(2.0)


def test_pair_slots():
    assert GD.pair_slots(1, 2) == [(0, 1)]
    assert GD.pair_slots(3, 7) == [(0, 3), (1, 4), (2, 5)]
    assert GD.pair_slots(64, 128)[-1] == (63, 127)
    for n, mb in ((1, 1), (2, 3), (65, 128), (5, 8)):
        with pytest.raises(ValueError):
            GD.pair_slots(n, mb)
    with pytest.raises(ValueError):
        GD.pair_slots(0, 8)


def test_records():
    r = GD.records(2.5, [(0, 3), (1, 4)], 6)
    assert r["scale"].tolist() == [2.5, 2.5, 0, 0, 0, 0] and r["partner"].tolist() == [3, 4, 0, 0, 0, 0]
    assert not GD.records(None, [(0, 1)], 2).view(np.uint8).any()                    # the all-zero record is neutral
    for bad in ([(0, 6)], [(6, 0)], [(2, 2)], [(-1, 0)]):
        with pytest.raises(ValueError):
            GD.records(2.0, bad, 6)


# --------------------------------------------------------------------------------------------------------- 3. layout and exports
def test_record_layout_matches_the_c_struct_and_the_built_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "aurora_hip.h")).read()
    fields = _lib.AurGuidance._fields_
    assert GD.RECORD.itemsize == 8 == ctypes.sizeof(_lib.AurGuidance)
    assert list(GD.RECORD.names) == [n for n, _ in fields]
    assert [GD.RECORD.fields[n][1] for n in GD.RECORD.names] == [getattr(_lib.AurGuidance, n).offset for n, _ in fields]
    assert re.search(r"typedef struct aur_guidance \{ float scale; int32_t partner; \} aur_guidance;", src)
    c = _lib.AurGuidance.from_buffer_copy(GD.records(7.5, [(1, 0)], 2)[1:2].tobytes())
    assert (c.scale, c.partner) == (7.5, 0)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in ("aur_slot_guidance", "aur_guidance_rows"):
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", src)
        assert getattr(raw, name) is not None                                       # AttributeError: the built library lacks it
    assert "guidance.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES
    assert '"dec_guid"' in open(os.path.join(ROOT, "aurora_amd", "csrc", "engine.hip")).read()


# -------------------------------------------------------------------------------------------------------------------- 4. the wiring
class _FakeEngine:
    dev, max_new_tokens, l, v, max_batch = "cpu", 64, {"hidden_size": 8, "num_hidden_layers": 2}, {}, 4

    def __init__(self):
        self.calls = []

    def generate(self, embeds, lens, n, eos_id=2, **kw):
        self.calls.append(kw)
        return [[1, 2, 3]]

    def text_embeds(self, ids):
        self.calls.append(dict(text_embeds=list(ids)))
        return torch.zeros(32, 8, dtype=torch.float16), len(ids)

    def caption_batch(self, clips, ratio, n, eos, **kw):
        self.calls.append(dict(kw, n_clips=len(clips)))
        return [[1] for _ in clips]


def test_llm_generate_honours_guidance_scale_and_needs_a_negative():
    from aurora_amd.model import _LLM
    e = _FakeEngine()
    llm = _LLM(e, 2)
    x = torch.zeros(1, 5, 8)
    for off in (dict(), dict(guidance_scale=None), dict(guidance_scale=1), dict(guidance_scale=1.0, negative_prompt_ids=[1, 2])):
        llm.generate(inputs_embeds=x, **off)
        assert e.calls == [{}]                                                       # the path of a call that never asked
        e.calls.clear()
    with pytest.raises(ValueError, match="negative"):
        llm.generate(inputs_embeds=x, guidance_scale=2)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            llm.generate(inputs_embeds=x, guidance_scale=bad, negative_prompt_ids=[1])
    assert e.calls == []
    llm.generate(inputs_embeds=x, guidance_scale=2, negative_prompt_ids=torch.tensor([[1, 5, 9]]))
    assert e.calls[0] == dict(text_embeds=[1, 5, 9])
    g = e.calls[1]["guidance"]
    assert g["scale"] == 2.0 and len(g["negative"]) == 1 and g["negative"][0][1] == 3
    e.calls.clear()
    llm.generate(inputs_embeds=x, guidance_scale=1.5, negative_inputs_embeds=torch.ones(1, 7, 8), repetition_penalty=1.2)
    g = e.calls[0]["guidance"]
    assert g["scale"] == 1.5 and g["negative"][0][1] == 7 and tuple(g["negative"][0][0].shape) == (32, 8)
    assert float(g["negative"][0][0][:7].float().min()) == 1.0 and not g["negative"][0][0][7:].any()
    assert e.calls[0]["logit_rules"]["repetition_penalty"] == pytest.approx(1.2)
    with pytest.raises(ValueError):
        llm.generate(inputs_embeds=x, guidance_scale=2, negative_inputs_embeds=torch.ones(1, 7, 9))


def test_aurora_model_caption_calls_pass_guidance_down_in_half_chunks():
    from aurora_amd.model import AuroraModel
    e = _FakeEngine()
    m = AuroraModel.__new__(AuroraModel)
    m.engine, m.slowfast = e, False
    m.visual_encoder = type("V", (), dict(visual_token_merge_ratio=0.5))()
    m.llm = type("L", (), dict(eos_token_id=2, config=e.l, _stop_tokenizer=None))()
    clips = [(torch.zeros(1, 3, 4, 4), [1, -200, 5])] * 5
    m.caption_batch(clips)
    assert [c["n_clips"] for c in e.calls] == [4, 1] and all("guidance" not in c for c in e.calls)
    e.calls.clear()
    m.caption_batch(clips, guidance_scale=1.0)
    assert [c["n_clips"] for c in e.calls] == [4, 1] and all("guidance" not in c for c in e.calls)
    e.calls.clear()
    m.caption_batch(clips, guidance_scale=3, negative_prompt=[1, 8, 9])
    assert [c["n_clips"] for c in e.calls] == [2, 2, 1]                              # max_batch // 2 guided clips per chunk
    assert all(c["guidance"] == dict(scale=3.0, negative_ids=[1, 8, 9]) for c in e.calls)
    e.calls.clear()
    m.caption_prompts(clips[0][0], [[1, -200, 5], [1, -200, 6]], guidance_scale=2)
    assert e.calls[0]["guidance"] == dict(scale=2.0, negative_ids=None) and e.calls[0]["share"] == [0, 0]
    with pytest.raises(ValueError, match="tokenizer"):
        m.caption_batch(clips, guidance_scale=2, negative_prompt="a photo")
    tok = lambda s: type("E", (), dict(input_ids=[1, 30, 31]))()                     # noqa: E731
    e.calls.clear()
    m.caption_batch(clips[:1], guidance_scale=2, negative_prompt="a photo", tokenizer=tok)
    assert e.calls[0]["guidance"]["negative_ids"] == [1, 30, 31]
    with pytest.raises(ValueError):
        m.caption_batch(clips, guidance_scale=-2)
    m.slowfast = True
    with pytest.raises(NotImplementedError):
        m.caption_batch(clips, guidance_scale=2)


def test_caption_stream_refuses_guidance_before_it_touches_anything():
    from aurora_amd.engine import AuroraCapEngine
    eng = AuroraCapEngine.__new__(AuroraCapEngine)                                   # no device, no state: the check comes first
    with pytest.raises(NotImplementedError, match="caption_stream"):
        next(eng.caption_stream([], 0.5, 4, guidance=dict(scale=2.0)))
    with pytest.raises(ValueError):
        next(eng.caption_stream([], 0.5, 4, guidance=dict(scale=-1.0)))


def test_engine_generate_checks_the_negatives_and_the_slots_before_it_touches_the_device():
    from aurora_amd.engine import AuroraCapEngine
    eng = AuroraCapEngine.__new__(AuroraCapEngine)
    eng.max_batch = 3
    with pytest.raises(ValueError, match="negative"):
        eng.generate([None, None], [4, 4], 8, guidance=dict(scale=2.0))
    with pytest.raises(ValueError, match="negative"):
        eng.generate([None, None], [4, 4], 8, guidance=dict(scale=2.0, negative=[(None, 3)]))
    with pytest.raises(ValueError, match="max_batch"):
        eng.generate([None, None], [4, 4], 8, guidance=dict(scale=2.0, negative=[(None, 3), (None, 3)]))


def test_the_adaptor_reads_guidance_from_the_generation_kwargs():
    from aurora_amd.lmms_plugin.models.auroracap_mi355x import gen_defaults, gen_guidance
    assert gen_guidance({}) is None and gen_guidance(dict(guidance_scale=1.0)) is None            # off by default
    assert gen_guidance(dict(guidance_scale=1.5)) == (1.5, None)
    assert gen_guidance(dict(guidance_scale=2, negative_prompt="a photo")) == (2.0, "a photo")
    for bad in (dict(guidance_scale=0), dict(guidance_scale="2"), dict(guidance_scale=2, negative_prompt=[1, 2])):
        with pytest.raises(ValueError):
            gen_guidance(bad)
        with pytest.raises(ValueError):
            gen_defaults(bad)
    assert gen_defaults(dict(guidance_scale=2.0))["guidance_scale"] == 2.0


def test_the_cli_has_the_two_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("inference_cli", os.path.join(ROOT, "inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--guidance_scale", "1.5", "--negative_prompt", "a photo"])
    assert a.guidance_scale == 1.5 and a.negative_prompt == "a photo"
    assert mod.build_parser().parse_args([]).guidance_scale is None

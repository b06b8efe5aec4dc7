"""Host plumbing of "one clip, several prompts" above the engine (no device): `AuroraCapEngine.caption_prompts` cuts the prompts into
chunks of max_batch with one share key per chunk, `AuroraModel.caption_batch / caption_prompts` hand order, streams and keys through,
a slow-fast model never shares, and `inference.py --extra_prompt` is a repeatable flag that changes nothing when absent."""
import importlib.util
import os
from types import SimpleNamespace

import torch

from aurora_amd import engine as E
from aurora_amd.model import AuroraModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeEngine:
    v, l = dict(hidden_size=8), dict(hidden_size=8)

    def __init__(self, max_batch):
        self.max_batch, self.max_new_tokens, self.calls = max_batch, 64, []

    def caption_batch(self, clips, ratio, max_new_tokens, eos_id=2, sampling=None, streams=None, share=None):
        self.calls.append(dict(n=len(clips), ratio=ratio, max_new=max_new_tokens, eos=eos_id, sampling=sampling,
                               streams=None if streams is None else list(streams), share=share, same_pixels=len({id(px) for px, _ in clips}) == 1))
        return [[len(ids), 0 if streams is None else list(streams)[i]] for i, (_, ids) in enumerate(clips)]

    caption_prompts = E.AuroraCapEngine.caption_prompts


PX = torch.zeros(2, 3, 4, 4)
PROMPTS = [[1, -200, 30] + [40] * k for k in (5, 1, 9, 3, 7)]


def test_engine_caption_prompts_chunks_by_max_batch_with_one_key_per_chunk():
    eng = FakeEngine(2)
    out = eng.caption_prompts(PX, PROMPTS, 0.5, 16, eos_id=None, sampling=dict(temperature=1.0), streams=[10, 11, 12, 13, 14])
    assert [x[0] for x in out] == [len(p) for p in PROMPTS]                    # prompt order
    assert [x[1] for x in out] == [10, 11, 12, 13, 14]                         # each prompt drew with its own stream
    assert [(c["n"], c["streams"], c["share"]) for c in eng.calls] == [(2, [10, 11], [0, 0]), (2, [12, 13], [0, 0]), (1, [14], [0])]
    assert all(c["same_pixels"] and c["eos"] is None and c["max_new"] == 16 and c["ratio"] == 0.5 for c in eng.calls)
    eng = FakeEngine(8)
    assert [x[1] for x in eng.caption_prompts(PX, PROMPTS, 0.5, 16)] == [0, 1, 2, 3, 4] and eng.calls[0]["sampling"] is None


def test_model_hands_keys_streams_and_order_through():
    eng = FakeEngine(3)
    m = AuroraModel(eng, eos_token_id=2)
    m.visual_encoder.reset_tome_r(0.3)
    out = m.caption_prompts(PX, [torch.tensor(p) for p in PROMPTS], max_new_tokens=1000)
    assert [x[0] for x in out] == [len(p) for p in PROMPTS]
    assert [(c["n"], c["share"], c["streams"]) for c in eng.calls] == [(3, [0, 0, 0], None), (2, [0, 0], None)]
    assert all(c["ratio"] == 0.3 and c["max_new"] == 64 and c["eos"] == 2 and c["same_pixels"] for c in eng.calls)      # capped at the engine's
    del eng.calls[:]
    clips = [(PX, p) for p in PROMPTS]
    m.caption_batch(clips, share=["a", "a", None, "b", "b"], sampling=dict(temperature=1.0), streams=[5, 6, 7, 8, 9])
    assert [(c["share"], c["streams"]) for c in eng.calls] == [(["a", "a", None], [5, 6, 7]), (["b", "b"], [8, 9])]
    del eng.calls[:]
    m.caption_batch(clips)                                                       # no keys: the engine is called as before
    assert all(c["share"] is None for c in eng.calls)


def test_slowfast_model_runs_the_prompts_one_at_a_time():
    eng = FakeEngine(4)
    m = AuroraModel(eng, eos_token_id=2, slowfast=True)
    m.visual_encoder.reset_tome_r(0.4)
    seen = []

    def forward(data, data_samples=None, mode="loss"):
        seen.append((m.visual_encoder.visual_token_merge_ratio, list(data["input_ids"][0]), tuple(data["pixel_values"].shape)))
        m.visual_encoder.visual_token_merge_ratio = 1.0                         # what the slow-fast forward leaves behind
        return {"inputs_embeds": torch.zeros(1, len(data["input_ids"][0]), 8)}
    m.forward = forward
    m.llm.generate = lambda inputs_embeds=None, **kw: torch.tensor([[inputs_embeds.shape[1], kw.get("stream", -1), int(kw["do_sample"])]])
    assert m.caption_prompts(PX, PROMPTS[:3], max_new_tokens=8) == [[len(p), -1, 0] for p in PROMPTS[:3]]
    assert seen == [(0.4, p, (1, 2, 3, 4, 4)) for p in PROMPTS[:3]] and not eng.calls          # the ratio is restored for every prompt
    assert m.visual_encoder.visual_token_merge_ratio == 0.4
    got = m.caption_prompts(PX, PROMPTS[:2], max_new_tokens=8, sampling=dict(temperature=0.7, top_p=0.9, top_k=5, seed=1), streams=[3, 4])
    assert got == [[len(PROMPTS[0]), 3, 1], [len(PROMPTS[1]), 4, 1]]


def test_inference_extra_prompt_flag():
    spec = importlib.util.spec_from_file_location("inference_cli", os.path.join(ROOT, "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    assert p.parse_args([]).extra_prompt == []
    a = p.parse_args(["--extra_prompt", "What moves?", "--prompt", "Describe.", "--extra_prompt", "Where is the camera?"])
    assert a.extra_prompt == ["What moves?", "Where is the camera?"] and a.prompt == "Describe."
    assert "seeded prompt" in p.format_help()

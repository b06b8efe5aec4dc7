"""CPU: scoring a given continuation - the numpy definition (aurora_amd/scoring.py) pinned to HF by tests/golden/g19_loglik.npz, the
oracle's teacher-forced logits on the same weights, the host-side layout of `loglikelihood_batch` (prompt ids, entry arrays, sharing
groups) and the adaptor's `loglikelihood` with injected fakes.  The kernels are covered by tests/test_gpu_score*.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from aurora_amd import engine as E
from aurora_amd import scoring
from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
from oracle import aurora_oracle as O
from tests.test_lmms_plugin import FakeModel, FakeTok, fake_pre
from tests.util import cfg_of, golden, sub


def g19_cases():
    g = golden("g19_loglik.npz")
    return g, [{k: g[f"c{c}.{k}"] for k in ("ids", "labels", "ctx_len", "loss", "argmax", "token_logprobs", "rows", "greedy")}
               for c in range(int(g["ncases"]))]


def g19_weights(g):
    flat, cfg = sub(g, "w."), cfg_of(g, "cfg")
    layers = []
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        layers.append({k[len(p):].replace("self_attn.", "").replace("mlp.", ""): v.float() for k, v in flat.items() if k.startswith(p)})
    return dict(layers=layers, **{k: flat[("model." if k != "lm_head.weight" else "") + k].float()
                                  for k in ("norm.weight", "embed_tokens.weight", "lm_head.weight")}), cfg


def test_g19_definition_equals_hf_loss_and_greedy_flag():
    """-sum_logprob / n == HF's `loss` (labels masked to -100 over the context) to 1e-5 and the greedy flag is HF's
    `(logits.argmax(-1)[ctx - 1 : -1] == continuation).all()`, from the fixture's own logits rows."""
    g, cases = g19_cases()
    assert "transformers" in cfg_of(g, "versions") and [bool(c["greedy"]) for c in cases] == [True, False, False]
    for c in cases:
        lc, ids = int(c["ctx_len"]), c["ids"]
        cont = ids[lc:].tolist()
        assert (c["labels"][:lc] == -100).all() and c["labels"][lc:].tolist() == cont
        total, greedy, lps = scoring.score_continuation(c["rows"], cont)
        assert abs(-total / len(cont) - float(c["loss"])) <= 1e-5
        np.testing.assert_allclose(lps, c["token_logprobs"], rtol=0, atol=1e-6)
        assert greedy == bool(c["greedy"]) == bool((c["argmax"][lc - 1:len(ids) - 1] == np.asarray(cont)).all())
        lp, am = scoring.score_rows(c["rows"], cont)
        assert am.tolist() == c["argmax"][lc - 1:len(ids) - 1].tolist() and abs(lp.sum() - total) < 1e-12
    # the corrupted continuation (case 2) differs from the greedy one (case 0) in one token and scores strictly lower there
    a, b = cases[0], cases[2]
    diff = np.nonzero(a["ids"] != b["ids"])[0]
    assert len(diff) == 1 and b["token_logprobs"][diff[0] - int(a["ctx_len"])] < a["token_logprobs"][diff[0] - int(a["ctx_len"])]


def test_g19_oracle_on_the_fixture_weights():
    """the oracle's llama_forward + lm_head over context + continuation[:-1] - the layout the engine scores - gives HF's loss and flag"""
    g, cases = g19_cases()
    lw, cfg = g19_weights(g)
    for c in cases:
        lc, ids = int(c["ctx_len"]), torch.from_numpy(c["ids"]).long()
        cont = ids[lc:].tolist()
        laid = E.loglik_ids(ids[:lc].tolist(), cont)
        assert laid == ids[:-1].tolist()
        h, _ = O.llama_forward(lw["embed_tokens.weight"][torch.tensor(laid)], lw, cfg, None, 0)
        rows = torch.nn.functional.linear(h[lc - 1:], lw["lm_head.weight"]).numpy()
        assert rows.shape[0] == len(cont)
        total, greedy, _ = scoring.score_continuation(rows, cont)
        assert abs(-total / len(cont) - float(c["loss"])) <= 1e-5
        assert greedy == bool(c["greedy"])


def test_score_row_definition_edges():
    V = 37
    lp, a = scoring.score_row(np.zeros(V, np.float32), 5)
    assert a == 0 and abs(lp + np.log(V)) < 1e-12                           # all equal: -log V, the first index
    l = np.zeros(V, np.float32)
    l[[9, 20]] = 3.0
    assert scoring.score_row(l, 20)[1] == 9                                 # an exact tie: the first index wins
    assert scoring.score_continuation(np.stack([l, l]), [9, 9])[1] is True and scoring.score_continuation(np.stack([l, l]), [9, 20])[1] is False
    big = np.full(V, 6.0e4, np.float32)
    big[3] = 6.0e4 + 2.0
    lp, a = scoring.score_row(big, 3)
    assert a == 3 and np.isfinite(lp) and lp < 0                            # the maximum is subtracted before exp
    assert scoring.score_continuation(np.zeros((0, V)), []) == (0.0, True, [])
    assert scoring.score_rows(np.zeros((2, V), np.float32), [-1, V]) [1].tolist() == [-1, -1]
    with pytest.raises(ValueError):
        scoring.score_row(l, V)


def test_layout_and_entry_arrays():
    ctx = [1, 17, -200, 18]
    # an empty continuation: the prompt is the context, there is nothing to score
    assert E.loglik_ids(ctx, []) == ctx
    with pytest.raises(ValueError):
        E.loglik_entries([40], [[]], 64)
    # one token: the prompt is the context alone, scored from its last position
    assert E.loglik_ids(ctx, [7]) == ctx
    rows, tg, spans = E.loglik_entries([40], [[7]], 64)
    assert rows.tolist() == [39] and tg.tolist() == [7] and spans == [(0, 1)] and rows.dtype == tg.dtype == np.int32
    # context 60 + 9 tokens: the prompt has 68 positions, rows 59 .. 67 cross the 64-row stride of a bucket of 64 -> stride 128
    cont = list(range(100, 109))
    assert E.loglik_ids(ctx, cont) == ctx + cont[:-1]
    assert E.prompt_stride(60 + 8, 64) == 128 and E.prefill_groups([68, 40], 8, 64) == [(0, 1, 128), (1, 1, 64)]
    rows, tg, spans = E.loglik_entries([60, 40], [cont, [7, 8]], 128)
    assert rows.tolist() == list(range(59, 68)) + [128 + 39, 128 + 40] and tg.tolist() == cont + [7, 8] and spans == [(0, 9), (9, 2)]
    with pytest.raises(ValueError):
        E.loglik_entries([60], [cont], 64)                                  # row 67 lies outside a stride of 64
    # behind a fork: rows are relative to the first position of the pass
    rows, _, _ = E.loglik_entries([70, 66], [[5, 6, 7], [9]], 32, pos0=64)
    assert rows.tolist() == [5, 6, 7, 32 + 1]
    with pytest.raises(ValueError):
        E.loglik_entries([64], [[5]], 32, pos0=64)                          # its first scored position lies in front of the fork
    with pytest.raises(ValueError):
        E.loglik_ids(ctx, [5, -200, 6])


def test_sharing_groups():
    n_kept, frames = 40, 2
    head = [1, 17, -200, 18, -200] + list(range(30, 50))                    # 2 * 40 visual rows + 23 text rows = 103 positions

    def plan(ctx, cont):
        return E.splice_rows(E.loglik_ids(ctx, cont), frames, n_kept)
    conts = [[60, 61, 62], [70, 71], [60, 61, 99, 98]]
    plans = [plan(head, c) for c in conts]
    ctx_lens = [p["seq_len"] - (len(c) - 1) for p, c in zip(plans, conts)]
    assert ctx_lens == [103] * 3
    # the same context and different continuations share: the fork is the last page boundary at or below position ctx_len - 1 = 102
    assert E.loglik_share_plan(plans, ctx_lens, ["a"] * 3) == [(0, [(1, 64), (2, 64)])]
    assert E.loglik_share_plan(plans, ctx_lens, ["a"] * 3, share=False) == [(0, []), (1, []), (2, [])]
    assert E.loglik_share_plan(plans, ctx_lens, ["a", "b", "b"]) == [(0, []), (1, [(2, 64)])]       # other pixels: a new head
    assert E.loglik_share_plan(plans, ctx_lens, [None] * 3) == [(0, []), (1, []), (2, [])]
    # a context that differs in front of the last visual row does not share
    other = plan([1, 19, -200, 18, -200] + list(range(30, 50)), [60])
    assert E.loglik_share_plan([plans[0], other], [103, 103], ["a", "a"]) == [(0, []), (1, [])]
    # a continuation that agrees with the head's beyond a page boundary still forks below its first scored row
    long_ctx = head + list(range(200, 225))                                 # 128 positions: the first scored row is 127
    same = [plan(long_ctx, [60, 61, 62, 63]), plan(long_ctx, [60, 61, 62, 77])]
    assert E.shared_prefix_rows(same[0], same[1]) == 131 and E.loglik_share_plan(same, [128, 128], ["a", "a"]) == [(0, [(1, 64)])]


class ScoreModel(FakeModel):
    def loglikelihood_batch(self, items):
        self.calls.append([(int(px.shape[0]), list(c), list(t)) for px, c, t in items])
        return [dict(logprob=-float(sum(t)), greedy=len(t) % 2 == 0, token_logprobs=[-float(x) for x in t], count=len(t)) for _, _, t in items]


def make(**kw):
    return P.AuroraCapMI355X(pretrained="unused", device="cpu", batch_size=3, _model=ScoreModel(), _tokenizer=FakeTok(), _preprocessor=fake_pre, **kw)


def test_adaptor_loglikelihood():
    tok = FakeTok()
    with pytest.raises(NotImplementedError):
        make().loglikelihood([])
    m = make(loglikelihood="True")
    docs = {i: np.zeros((2 + i % 2, 8, 8, 3), np.uint8) for i in range(3)}
    m.task_dict = {"mc": {"test": docs}}
    answers = {0: ["yes", "no"], 1: ["cat", "a dog", "bird"], 2: ["x"]}
    reqs, want = [], []
    for k in range(3):                                                      # candidates of the documents interleaved: 0 1 2 0 1 1
        for d in range(3):
            if k < len(answers[d]):
                a = answers[d][k]
                reqs.append(SimpleNamespace(args=(f"question {d}?", a if d != 1 else (lambda doc, a=a: a), lambda doc: [doc], d, "mc", "test")))
                q = P.question_with_image_tokens(f"question {d}?", 2 + d % 2)
                ctx = P.tokenizer_image_token(P.conv_prompt(q), tok)
                full = P.tokenizer_image_token(P.conv_prompt(q) + " " + a + "</s>", tok)
                assert full[:len(ctx)] == ctx
                want.append((d, ctx, full[len(ctx):]))
    out = m.loglikelihood(reqs)
    assert m.model.visual_encoder.ratio == 0.4
    assert out == [(-float(sum(t)), len(t) % 2 == 0) for _, _, t in want]    # (sum, greedy) in REQUEST order
    seen = [it for call in m.model.calls for it in call]
    assert [len(c) for c in m.model.calls] == [3, 3]                        # chunks of batch_size
    # equal (task, split, doc, context) are neighbours, in order of first appearance; each got ITS context / continuation split
    assert [(f, c, t) for f, c, t in seen] == [(2 + d % 2, ctx, t) for d0 in range(3) for d, ctx, t in want if d == d0]
    assert m.loglikelihood_detail(reqs[:1])[0]["count"] == len(want[0][2])
    assert P.loglik_split("q", "", tok)[1] == []                            # an empty answer: nothing to score

"""GPU: `AuroraCapEngine.loglikelihood_batch` on the tiny ViT + projector + Llama of test_projector_splice_and_whole_path - scoring the
engine's own caption against its decode logits, the shared-prefix route against the unshared one, and a corrupted continuation."""
import pytest
import torch

from tests.parity_bounds import LOGIT_TOL
from tests.test_gpu_llm import LLM_CFGS
from tests.util import rand_llm_weights, rand_proj_weights, rand_vit_weights

pytestmark = pytest.mark.gpu

VCFG = dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=4, intermediate_size=128, patch_size=14, image_size=56,
            hidden_act="quick_gelu", layer_norm_eps=1e-5)
IDS = [1, 17, -200, 18, -200, 19, -200, 20, 21, 22]
NEW = 8


@pytest.fixture(scope="module")
def case():
    """the engine, a clip, its greedy caption of 8 tokens and the decode path's logits row behind every one of them"""
    from aurora_amd.engine import AuroraCapEngine
    lcfg = LLM_CFGS["hd32"]
    w = {"vit": rand_vit_weights(VCFG, 1), "projector": rand_proj_weights(64, lcfg["hidden_size"], 2), "llm": rand_llm_weights(lcfg, 3)}
    eng = AuroraCapEngine({"vit": VCFG, "llm": lcfg}, w, max_frames=3, max_batch=3, max_ctx=256, max_new_tokens=16)
    px = torch.randn(3, 3, 56, 56, generator=torch.Generator().manual_seed(76)).half().float()
    vis = eng.vit_encode(px, eng.tome_r(0.5))
    emb, L = eng.project_splice(vis, IDS)
    eng.begin_batch(1, NEW, None)
    eng.prefill(0, emb, L)
    rows = [eng.logits()[0].cpu()]
    for _ in range(NEW - 1):
        eng.decode(1)
        rows.append(eng.logits()[0].cpu())
    caption = eng.outputs()[0]
    assert len(caption) == NEW and caption == eng.caption_ids(px, IDS, 0.5, NEW, eos_id=None)
    yield eng, px, caption, torch.stack(rows)
    eng.close()


def test_scoring_the_generated_caption(case):
    """token_logprobs within 4 * LOGIT_TOL * max|logit| of the log-softmax of the decode logits: the prefill path and the decode path
    are each within LOGIT_TOL * max|logit| of the oracle's logits, and a log-probability is 2-Lipschitz in the sup norm of its row."""
    eng, px, caption, rows = case
    r = eng.loglikelihood_batch([(px, IDS, caption)], 0.5)[0]
    assert r["count"] == NEW and len(r["token_logprobs"]) == NEW
    want = torch.log_softmax(rows.double(), -1)
    bound = 4 * LOGIT_TOL * rows.abs().max().item()
    total = 0.0
    for j, t in enumerate(caption):
        err = abs(r["token_logprobs"][j] - want[j, t].item())
        print(f"caption token {j}: |dlp| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, j
        total += r["token_logprobs"][j]
    assert r["logprob"] == total
    top2 = rows.topk(2, -1).values
    if (top2[:, 0] - top2[:, 1]).min().item() > 2 * bound:                   # every pick clear of the tolerance: the caption is greedy here too
        assert r["greedy"] is True
    assert eng.loglikelihood_batch([(px, IDS, [])], 0.5) == [dict(logprob=0.0, greedy=True, token_logprobs=[], count=0)]


def test_shared_prefix_route_is_bitwise_the_unshared_one(case):
    """three continuations of one clip and one context of 84+ positions: the fork (64) lies below the first scored row, the siblings copy
    the head's first page and are scored in one pass at pos0 = 64 - the same bits, and one ViT pass instead of three"""
    eng, px, caption, _ = case
    ctx = IDS + list(range(30, 90))
    conts = [caption[:4], [5, 6, 7, 8, 9, 10], caption[:2] + [40, 41, 42]]
    items = [(px, ctx, c) for c in conts]
    out, vit = {}, {}
    for share in (True, False):
        eng.profile(True)
        out[share] = eng.loglikelihood_batch(items, 0.5, share=share)
        vit[share] = eng.profile_read("vit")[1]
        eng.profile(False)
    assert (vit[True], vit[False]) == (1, 3)
    for a, b, c in zip(out[True], out[False], conts):
        assert a["token_logprobs"] == b["token_logprobs"] and a["logprob"] == b["logprob"] and a["greedy"] == b["greedy"]
        assert a["count"] == len(c)
    assert out[True][0]["token_logprobs"][:2] == out[True][2]["token_logprobs"][:2]      # the same leading tokens: the same values
    # each item alone is the same again, and so is a different order (another head)
    alone = [eng.loglikelihood_batch([it], 0.5)[0] for it in items]
    assert alone == out[True] and eng.loglikelihood_batch(items[::-1], 0.5)[::-1] == out[True]
    with pytest.raises(ValueError):
        eng.loglikelihood_batch([(px, ctx + list(range(30, 90)) * 3, [5])], 0.5)      # beyond max_ctx


def test_a_corrupted_continuation(case):
    eng, px, caption, rows = case
    k = 4
    bad = list(caption)
    bad[k] = int(rows[k].argmin())                                          # the least likely token of that step: certainly not the argmax
    good, worse = eng.loglikelihood_batch([(px, IDS, caption), (px, IDS, bad)], 0.5)
    assert worse["greedy"] is False
    assert worse["token_logprobs"][k] < good["token_logprobs"][k]
    assert worse["token_logprobs"][:k] == good["token_logprobs"][:k]        # the rows in front of it saw the same tokens

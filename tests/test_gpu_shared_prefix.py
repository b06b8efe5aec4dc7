"""GPU: several prompts about one clip (`caption_batch(share=)`, `caption_prompts`, `caption_stream(share_key=)`) give every
(clip, prompt) exactly the ids `caption_ids` gives it alone, while the ViT runs once per clip.  List equality, no tolerance.

The clips: 6 frames of 56 x 56 at ratio 0.5 keep 10 visual rows per frame, so BOS + 6 x (10 visual rows + a separator) = 67 rows are
common to every prompt about a clip: prompt A and B go on with the same 70 text tokens (B forks off A at row 128), C with 40 of them
(it forks at row 64, inside the last frame's visual rows) - different forks and different lengths in one batch."""
import pytest
import torch

from tests.test_gpu_llm import LLM_CFGS
from tests.test_gpu_prefill_var import count_calls

pytestmark = pytest.mark.gpu

N, RATIO, FRAMES = 12, 0.5, 6
COMMON = [200 + j for j in range(70)]
TAILS = {"A": COMMON + [100, 101, 102, 103, 104], "B": COMMON + [110 + j for j in range(21)], "C": COMMON[:40] + [140, 141, 142]}


def engine(max_batch, spare=0, prefix_cache=0):
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_caption_batch import VCFG, weights
    return AuroraCapEngine({"vit": VCFG, "llm": LLM_CFGS["hd32"]}, weights(), max_frames=FRAMES, max_batch=max_batch, max_ctx=512,
                           max_new_tokens=N, spare_slots=spare, prefix_cache=prefix_cache)


def requests(order):
    """[(clip index, prompt name)] -> clips, share keys"""
    gen = torch.Generator().manual_seed(90)
    px = [torch.randn(FRAMES, 3, 56, 56, generator=gen).half().cuda() for _ in range(3)]
    return [(px[c], [1] + [-200, 30] * FRAMES + TAILS[p]) for c, p in order], [("clip", c) for c, _ in order]


ADJACENT = [(c, p) for c in range(3) for p in "ABC"]
INTERLEAVED = [(c, p) for p in "ABC" for c in range(3)]


@pytest.fixture(scope="module")
def alone():
    """every (clip, prompt) through the existing single-clip path, once for the whole module"""
    eng = engine(1)
    try:
        cs, _ = requests(ADJACENT)
        return {cp: eng.caption_ids(px, ids, RATIO, N, eos_id=None) for cp, (px, ids) in zip(ADJACENT, cs)}
    finally:
        eng.close()


def test_the_prompts_fork_where_the_docstring_says():
    from aurora_amd.engine import share_fork, splice_rows
    plans = {p: splice_rows([1] + [-200, 30] * FRAMES + TAILS[p], FRAMES, 10) for p in "ABC"}
    assert plans["A"]["vis_end"] == 66 and share_fork(plans["A"], plans["B"]) == 128 and share_fork(plans["A"], plans["C"]) == 64
    assert len({plans[p]["seq_len"] for p in "ABC"}) == 3


@pytest.mark.parametrize("order", [ADJACENT, INTERLEAVED], ids=["adjacent", "interleaved"])
def test_caption_batch_shares_the_vit_pass_and_the_prefix(alone, order):
    cs, keys = requests(order)
    eng = engine(9)
    try:
        vit, ext, cp = count_calls(eng, "vit_encode"), count_calls(eng, "extend_batch"), count_calls(eng, "kv_copy_prefix")
        got = eng.caption_batch(cs, RATIO, N, eos_id=None, share=keys)
        assert got == [alone[cp_] for cp_ in order]
        assert len(vit) == 3 and len(ext) == len(cp) == 6          # B and C fork at different rows: a pass each
        assert sorted({c[0][3] for c in cp}) == [64, 128]
        assert eng.caption_batch(cs, RATIO, N, eos_id=None) == got and len(vit) == 3 + 9      # share=None: the path of before
        assert len(ext) == len(cp) == 6
    finally:
        eng.close()


def test_neighbouring_siblings_of_one_fork_share_a_pass_and_caption_prompts(alone):
    cs, _ = requests([(1, "A"), (1, "B"), (1, "B"), (1, "A"), (1, "C")])
    eng = engine(5)
    try:
        vit, ext, cp = count_calls(eng, "vit_encode"), count_calls(eng, "extend_batch"), count_calls(eng, "kv_copy_prefix")
        got = eng.caption_prompts(cs[0][0], [ids for _, ids in cs], RATIO, N, eos_id=None)
        assert got == [alone[(1, p)] for p in "ABBAC"]
        assert len(vit) == 1
        # B, B and the repeated A (142 rows: it forks at 128 too, keeping rows of its own): one copy with three destinations, one pass
        assert [(c[0][2], c[0][3]) for c in cp] == [(3, 128), (1, 64)]
        assert [c[0][1] for c in ext] == [3, 1]
        sampled = dict(temperature=0.8, top_k=20, top_p=0.9, seed=3)
        want = [eng.caption_ids(cs[0][0], ids, RATIO, N, eos_id=None, sampling=sampled, stream=7 + k) for k, (_, ids) in enumerate(cs)]
        assert eng.caption_prompts(cs[0][0], [ids for _, ids in cs], RATIO, N, eos_id=None, sampling=sampled, streams=range(7, 12)) == want
    finally:
        eng.close()


@pytest.mark.parametrize("overlap,spare,prefix_cache,front_graph", [(False, 1, 1, False), (False, 2, 2, False), (True, 3, 1, False),
                                                                    (True, 4, 2, False), (True, 3, 1, True)])
def test_caption_stream_with_holders(alone, overlap, spare, prefix_cache, front_graph):
    eng = engine(3, spare, prefix_cache)
    try:
        passes = count_calls(eng, "_front_end_replay" if front_graph else "vit_encode")
        cs, keys = requests(ADJACENT)
        kw = dict(eos_id=None, check_every=4, overlap=overlap, share_key=lambda i: keys[i], **(dict(front_graph=front_graph) if overlap else {}))
        assert dict(eng.caption_stream(cs, RATIO, N, **kw)) == {i: alone[cp] for i, cp in enumerate(ADJACENT)}
        assert len(passes) == 3                                    # one ViT pass per clip: the first prompt's
        # siblings interleaved: with 3 clips in turn, a cache of 1 or 2 least-recently-used holders never holds the clip that comes
        # next - every request misses and runs its own ViT pass (9), and the ids are still those of each request alone
        del passes[:]
        cs, keys = requests(INTERLEAVED)
        assert dict(eng.caption_stream(cs, RATIO, N, **kw)) == {i: alone[cp] for i, cp in enumerate(INTERLEAVED)}
        assert len(passes) == 9
        if not front_graph:
            del passes[:]                                          # no keys: the path of before
            assert dict(eng.caption_stream(cs, RATIO, N, **{k: v for k, v in kw.items() if k != "share_key"})) == \
                {i: alone[cp] for i, cp in enumerate(INTERLEAVED)}
            assert len(passes) == 9
    finally:
        eng.close()


def test_fallbacks_take_the_unshared_path():
    """two frames: 23 common rows and short tails - less than a page is shared, so keyed clips are prefilled as always; and a call
    without keys never reaches the new entry points"""
    gen = torch.Generator().manual_seed(91)
    px = torch.randn(2, 3, 56, 56, generator=gen).half().cuda()
    cs = [(px, [1] + [-200, 30] * 2 + [100 + j for j in range(t)]) for t in (3, 9, 5)]
    eng = engine(3, 1, 1)
    try:
        want = [eng.caption_ids(p, ids, RATIO, N, eos_id=None) for p, ids in cs]
        new = [count_calls(eng, n) for n in ("kv_copy_prefix", "extend_batch", "extend_stage", "extend_commit")]
        vit = count_calls(eng, "vit_encode")
        assert eng.caption_batch(cs, RATIO, N, eos_id=None, share=["k"] * 3) == want
        assert dict(eng.caption_stream(cs, RATIO, N, eos_id=None, check_every=4, overlap=False, share_key=lambda i: "k")) == dict(enumerate(want))
        assert len(vit) == 6 and not any(new)
        assert eng.caption_batch(cs, RATIO, N, eos_id=None) == want
        assert dict(eng.caption_stream(cs, RATIO, N, eos_id=None, check_every=4, overlap=False)) == dict(enumerate(want))
        assert not any(new)
        with pytest.raises(ValueError):
            eng.caption_batch(cs, RATIO, N, eos_id=None, share=["k"] * 2)
    finally:
        eng.close()
    eng = engine(3)
    try:
        with pytest.raises(ValueError):                            # no holder sequences
            list(eng.caption_stream(cs, RATIO, N, eos_id=None, share_key=lambda i: "k"))
    finally:
        eng.close()
    from aurora_amd.engine import AuroraCapEngine
    with pytest.raises(ValueError):
        AuroraCapEngine({"vit": None, "llm": None}, {}, spare_slots=1, prefix_cache=2)

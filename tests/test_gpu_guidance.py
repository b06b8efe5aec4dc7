"""Classifier-free guidance on the GPU through the decode path: a guided request is a pair of KV slots that decode
in lock-step; the leader's pick comes from the contrast of the two rows.
  1. teacher-forced against the fp32 oracle's two rows combined by `aurora_amd.guidance.apply`, under the margin rule;
  2. the partner holds the leader's ids, length and finished flag after every run;
  3. the ids do not depend on batch, slot order, neighbours or graph capture, and an unguided neighbour is not touched;
  4. scale 1 is the plain call; 5. log-probabilities are those of the model's conditional row; 6. EOS and budgets end both;
  7. sampling; 8. the logit rules come after guidance; 9. caption_ids / caption_batch.
The kernels alone are in tests/test_gpu_guidance_rows.py, the definition against transformers in tests/test_guidance_host.py."""
import numpy as np
import pytest
import torch

from aurora_amd import guidance as GD
from aurora_amd import logit_rules as LR
from aurora_amd import sampling as S
from aurora_amd._lib import AuroraHipError
from tests import guidance_ref as R
from tests.guidance_cases import PAIRS, guided_margin_check, pair_embeds
from tests.parity_bounds import LOGIT_TOL
from tests.test_gpu_llm import LLM_CFGS, make_engine, padded, teacher_forced_logits

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lead(emb, partner):
    return dict(kind="lead", emb=emb, partner=partner)


def part(emb):
    return dict(kind="part", emb=emb)


def plain(emb):
    return dict(kind="plain", emb=emb)


IDLE = dict(kind="idle")


def run(e, slots, n_new, g, eos=None, stepwise=False, after=0, lp=None):
    """Slots as laid out by the caller: leaders name their partners' slots, idle slots are retired.  Partners and unguided slots are
    prefilled first.  -> dict(ids per slot, lens, fin, logits per step [step][slot, vocab] when stepwise).  after: further decode
    steps behind the n_new - 1 a full row needs."""
    B = len(slots)
    e._guidance_on()
    if lp is not None:
        e._logprobs_on(lp)
    e.begin_batch(B, n_new, eos)
    recs = np.zeros(B, GD.RECORD)
    for b, s in enumerate(slots):
        if s["kind"] == "lead":
            recs[b] = (g, s["partner"])
    e.slot_guidance(0, recs)
    for first in (False, True):
        for b, s in enumerate(slots):
            if s["kind"] == "idle":
                if not first:
                    e.slot_retire(b)
            elif (s["kind"] == "lead") == first:
                e.prefill(b, padded(s["emb"]), s["emb"].shape[0])
    rows = [e.logits().cpu().numpy()] if stepwise else None
    if stepwise:
        for _ in range(n_new - 1 + after):
            e.decode(1)
            rows.append(e.logits().cpu().numpy())
    elif n_new - 1 + after > 0:
        e.decode(n_new - 1 + after)
    lens, fin = e.slot_state()
    return dict(ids=e.outputs(), lens=lens.tolist(), fin=fin.tolist(), rows=rows)


def assert_partners_follow(slots, out):
    for b, s in enumerate(slots):
        if s["kind"] == "lead":
            p = s["partner"]
            assert out["ids"][p] == out["ids"][b] and out["lens"][p] == out["lens"][b] and out["fin"][p] == out["fin"][b], (b, p)


@pytest.fixture(scope="module", params=["hd32", "hd128"])
def ctx(request):
    cfg = LLM_CFGS[request.param]
    e, w = make_engine(cfg, 5, max_batch=18, max_new=24)
    yield request.param, cfg, e, w
    e.close()


# ---------------------------------------------------------------------------------------------- 1 / 2. against the oracle's two rows
@pytest.mark.parametrize("g", [1.5, 3.0])
def test_guided_ids_are_the_pick_from_the_oracles_two_rows(ctx, g):
    name, cfg, e, w = ctx
    for seed, Lc, Ln, n_new in PAIRS[name]:
        c, u = pair_embeds(cfg, seed, Lc, Ln)
        slots = [lead(c, 1), part(u)]
        out = run(e, slots, n_new, g)
        assert_partners_follow(slots, out)
        ids = out["ids"][0]
        assert len(ids) == n_new and out["fin"] == [1, 1]
        skipped = guided_margin_check(ids, c, u, w, cfg, g, tag=f"guidance/guided_row_margin[{name}]")
        assert 4 * skipped <= n_new, (seed, skipped)
        # the same call through generate(guidance=): leaders' results alone
        got = e.generate([padded(c)], [Lc], n_new, eos_id=None, guidance=dict(scale=g, negative=[(padded(u), Ln)]))
        assert got == [ids]


# ------------------------------------------------------------------------------------------------------------ 3. bitwise properties
def test_ids_do_not_depend_on_batch_slot_order_or_neighbours(ctx):
    name, cfg, e, w = ctx
    g, n_new = 2.0, 16
    (ca, ua), (cb, ub), (cc, uc) = [pair_embeds(cfg, s, Lc, Ln) for s, Lc, Ln, _ in PAIRS[name][:3]]
    x = pair_embeds(cfg, 99, 57, 9)[0]
    alone = []
    for c, u in ((ca, ua), (cb, ub), (cc, uc)):
        slots = [lead(c, 1), part(u)]
        out = run(e, slots, n_new, g)
        assert_partners_follow(slots, out)
        alone.append(out["ids"][0])
    assert len({tuple(a) for a in alone}) == 3
    # three pairs and one unguided slot in one batch: partners above and below their leaders
    slots = [lead(ca, 4), part(ub), lead(cb, 1), plain(x), part(ua), part(uc), lead(cc, 5)]
    big = run(e, slots, n_new, g)
    assert_partners_follow(slots, big)
    assert [big["ids"][0], big["ids"][2], big["ids"][6]] == alone
    # the other order, and a pair across the 16-slot fragment boundary with idle slots around it
    out = run(e, [part(ua), lead(ca, 0)], n_new, g)
    assert out["ids"][1] == alone[0] and out["ids"][0] == alone[0]
    slots = [IDLE] * 15 + [part(ub), lead(cb, 15), plain(x)]
    far = run(e, slots, n_new, g)
    assert_partners_follow(slots, far)
    assert far["ids"][16] == alone[1]
    # the unguided slot beside the pairs: exactly the plain call's ids, from an engine that never heard of guidance
    e2, _ = make_engine(cfg, 5, max_batch=1, max_new=24)
    try:
        want = e2.generate([padded(x)], [x.shape[0]], n_new, eos_id=None)[0]
    finally:
        e2.close()
    assert big["ids"][3] == want
    assert far["ids"][17] == want
    assert e.generate([padded(x)], [x.shape[0]], n_new, eos_id=None)[0] == want          # and the plain call on the guided engine
    # guidance is not a no-op here
    assert alone[0] != e.generate([padded(ca)], [ca.shape[0]], n_new, eos_id=None)[0]


def test_captured_steps_equal_eager_steps():
    cfg = LLM_CFGS["hd32"]
    seed, Lc, Ln, n_new = PAIRS["hd32"][0]
    c, u = pair_embeds(cfg, seed, Lc, Ln)
    outs = []
    for use_graph in (False, True):
        e, _ = make_engine(cfg, 5, max_batch=4, use_graph=use_graph)
        try:
            outs.append(e.generate([padded(c), padded(u)], [Lc, Ln], n_new, eos_id=None,
                                   guidance=dict(scale=3.0, negative=[(padded(u), Ln), (padded(c), Lc)])))
        finally:
            e.close()
    assert outs[0] == outs[1] and outs[0][0] != outs[0][1]


# ------------------------------------------------------------------------------------------------------------------- 4. scale 1
def test_scale_one_is_the_plain_call_and_leaves_the_option_off():
    cfg = LLM_CFGS["hd32"]
    seed, Lc, Ln, n_new = PAIRS["hd32"][0]
    c, u = pair_embeds(cfg, seed, Lc, Ln)
    e, _ = make_engine(cfg, 5, max_batch=2)
    try:
        want = e.generate([padded(c)], [Lc], n_new, eos_id=None)
        for off in (None, dict(scale=1.0, negative=[(padded(u), Ln)]), dict(scale=None)):
            assert e.generate([padded(c)], [Lc], n_new, eos_id=None, guidance=off) == want
        assert e._guid_mode is False
        e.begin_batch(2, 4, None)
        with pytest.raises(AuroraHipError):                                           # the option is 0: the ctx holds no records to set
            e.slot_guidance(0, GD.records(2.0, [(0, 1)], 2))
        with pytest.raises(AuroraHipError):
            e.microbench("dec_guid", 1)
        with pytest.raises(ValueError):                                               # a pair needs two slots
            e.generate([padded(c), padded(c)], [Lc, Lc], 4, guidance=dict(scale=2.0, negative=[(padded(u), Ln)] * 2))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 5. log-probabilities
def test_logprobs_are_those_of_the_models_conditional_row(ctx):
    name, cfg, e, w = ctx
    seed, Lc, Ln, _ = PAIRS[name][1]
    g, n_new = 3.0, 12
    c, u = pair_embeds(cfg, seed, Lc, Ln)
    slots = [part(u), lead(c, 0)]
    base = run(e, slots, n_new, g)
    try:
        out = run(e, slots, n_new, g, stepwise=True, lp=2)
        rec, lp, tid, tlp = e.token_logprob_state()
    finally:
        e.logprobs_off()
    assert out["ids"] == base["ids"] and rec[1] == n_new                               # the ids are unchanged by asking
    ids = out["ids"][1]
    ref_c, ref_u = teacher_forced_logits(c, ids, w, cfg), teacher_forced_logits(u, ids, w, cfg)
    differs = 0
    for i in range(n_new):
        rows = torch.from_numpy(out["rows"][i]).cuda()
        want, _ = e.score_rows(rows[1:2].contiguous(), [ids[i]])
        assert bits(lp[1, i]) == bits(want[0]), i                                      # bitwise score_rows of the model's row
        # and the rows the engine shows between steps are the model's, of both slots - not the guided row
        for slot, ref in ((1, ref_c), (0, ref_u)):
            assert float(np.abs(out["rows"][i][slot] - ref[i].numpy()).max()) <= LOGIT_TOL * float(ref.abs().max()), (i, slot)
        differs += int(np.argmax(out["rows"][i][1]) != ids[i])
        assert tid[1, i, 0] == int(np.argmax(out["rows"][i][1]))                       # rank 0 is the model's own first choice
    assert differs > 0                                                                 # guidance did pick against the model's argmax


# ------------------------------------------------------------------------------------------------------------------- 6. EOS, budgets
def test_eos_and_budgets_end_both_slots(ctx):
    name, cfg, e, w = ctx
    seed, Lc, Ln, _ = PAIRS[name][2]
    g, n_new = 2.0, 16
    c, u = pair_embeds(cfg, seed, Lc, Ln)
    slots = [lead(c, 1), part(u)]
    free = run(e, slots, n_new, g)["ids"][0]
    k = next(i for i in range(3, n_new) if free.index(free[i]) == i)                   # a token whose first occurrence is step k
    out = run(e, slots, n_new, g, eos=free[k])
    assert out["ids"][0] == free[:k + 1] and out["ids"][1] == free[:k + 1] and out["lens"] == [k + 1] * 2 and out["fin"] == [1, 1]
    more = run(e, slots, n_new, g, eos=free[k], after=5)                               # further steps change nothing
    assert more["ids"] == out["ids"] and more["lens"] == out["lens"] and more["fin"] == out["fin"]
    # a budget of the leader's own ends both
    got = e.generate([padded(c)], [Lc], n_new, eos_id=None, stop=[dict(max_new_tokens=5)],
                     guidance=dict(scale=g, negative=[(padded(u), Ln)]))
    lens, fin = e.slot_state()
    assert got == [free[:5]] and e.outputs() == [free[:5]] * 2 and lens.tolist() == [5, 5] and fin.tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------------------------------ 7. sampling
def test_sampled_guided_ids_depend_on_seed_and_stream_not_on_the_slot(ctx):
    name, cfg, e, w = ctx
    (ca, ua), (cb, ub) = [pair_embeds(cfg, s, Lc, Ln) for s, Lc, Ln, _ in PAIRS[name][:2]]
    sp = dict(temperature=0.8, top_k=20, seed=3)
    neg = lambda x: (padded(x), x.shape[0])                                            # noqa: E731
    kw = dict(eos_id=None, sampling=sp)
    one = e.generate([padded(cb)], [cb.shape[0]], 16, streams=[5], guidance=dict(scale=2.0, negative=[neg(ub)]), **kw)[0]
    two = e.generate([padded(ca), padded(cb)], [ca.shape[0], cb.shape[0]], 16, streams=[9, 5],
                     guidance=dict(scale=2.0, negative=[neg(ua), neg(ub)]), **kw)
    assert two[1] == one
    other = e.generate([padded(cb)], [cb.shape[0]], 16, streams=[6], guidance=dict(scale=2.0, negative=[neg(ub)]), **kw)[0]
    assert other != one
    greedy = e.generate([padded(cb)], [cb.shape[0]], 16, eos_id=None, guidance=dict(scale=2.0, negative=[neg(ub)]))[0]
    assert greedy != one
    lens, fin = e.slot_state()
    assert e.outputs()[1] == greedy and lens.tolist() == [16, 16]


# --------------------------------------------------------------------------------------------------------------------- 8. logit rules
def test_logit_rules_come_after_guidance(ctx):
    name, cfg, e, w = ctx
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    g = 1.5
    for seed, Lc, Ln, n_new in PAIRS[name][:2]:
        c, u = pair_embeds(cfg, seed, Lc, Ln)
        ids = e.generate([padded(c)], [Lc], n_new, eos_id=None, logit_rules=rules, guidance=dict(scale=g, negative=[(padded(u), Ln)]))[0]
        assert e.outputs()[1] == ids
        assert all((ids[i], ids[i + 1]) not in {(ids[j], ids[j + 1]) for j in range(i)} for i in range(len(ids) - 1))   # no 2-gram twice
        skipped = guided_margin_check(ids, c, u, w, cfg, g, rules=LR.check_logit_rules(rules),
                                      tag=f"guidance/guided_row_margin_with_rules[{name}]")
        assert 4 * skipped <= n_new, (seed, skipped)


# ---------------------------------------------------------------------------------------------------------------- 9. the caption calls
def test_caption_ids_and_caption_batch_under_guidance():
    from tests.test_gpu_caption_batch import build, clips
    eng = build(max_batch=6)
    try:
        cs = clips(3, 3)
        g = dict(scale=2.0)
        singles = []
        for px, ids in cs:
            got = eng.caption_ids(px, ids, 0.5, 12, eos_id=None, guidance=g)
            # by hand: the two spliced prefixes into generate - the default negative is the prompt without its image markers
            vis = eng.vit_encode(px, eng.tome_r(0.5, px.shape[-2], px.shape[-1]))
            emb, L = eng.project_splice(vis, ids)
            nemb, Ln = eng.text_embeds([t for t in ids if t != -200])
            assert Ln == sum(1 for t in ids if t != -200) and L > Ln
            want = eng.generate([emb], [L], 12, eos_id=None, guidance=dict(scale=2.0, negative=[(nemb, Ln)]))[0]
            assert got == want
            assert got != eng.caption_ids(px, ids, 0.5, 12, eos_id=None)
            singles.append(got)
        assert eng.caption_batch(cs, 0.5, 12, eos_id=None, guidance=g) == singles
        # a negative that keeps its markers is spliced over the same kept visual rows: the prompt as its own negative changes nothing
        px, ids = cs[0]
        assert eng.caption_ids(px, ids, 0.5, 12, eos_id=None, guidance=dict(scale=2.0, negative_ids=ids)) == \
            eng.caption_ids(px, ids, 0.5, 12, eos_id=None)
        # one negative for every prompt, in chunks of max_batch // 2
        same = eng.caption_prompts(px, [ids, ids[:-1] + [50], ids + [51], ids + [52, 53]], 0.5, 8, eos_id=None,
                                   guidance=dict(scale=2.0, negative_ids=[1, 40, 41]))
        for q, r in zip([ids, ids[:-1] + [50], ids + [51], ids + [52, 53]], same):
            assert r == eng.caption_ids(px, q, 0.5, 8, eos_id=None, guidance=dict(scale=2.0, negative_ids=[1, 40, 41]))
        with pytest.raises(ValueError):
            eng.caption_batch(clips(4, 4), 0.5, 4, eos_id=None, guidance=g)            # 4 guided clips need 8 slots
        with pytest.raises(NotImplementedError):
            next(eng.caption_stream(iter(cs), 0.5, 4, eos_id=None, guidance=g))
    finally:
        eng.close()

"""Logit rules on the GPU: repetition penalty, no-repeat n-gram and min-new-tokens ahead of the token pick.
  1 / 2. the kernels alone (aur_logit_rules_rows) against `aurora_amd.logit_rules.apply`, bit for bit, and the restore;
  3 / 6. an audit of the engine on its own logits: every emitted token is the pick from the processed row, the rows the engine
         shows between steps are the model's, and the recorded log-probabilities are those of the unmodified rows;
  4.     the properties a caller asks for; 5. the ids do not depend on batch, slot, neighbours, bank, graph or slot reuse;
  7.     llm.generate, the lmms-eval adaptor and the CLI.
The definition itself is checked against transformers in tests/test_logit_rules_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from aurora_amd import logit_rules as LR
from aurora_amd import sampling as S
from tests.logit_rules_cases import EOS, cases, make_row
from tests.test_gpu_llm import LLM_CFGS, make_engine, padded
from tests.util import golden, observe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 4.0 * float(golden("g18_sampling.npz")["f32_cdf_dev"])          # the sampled pick's bound (tests/test_gpu_sampling.py)
CFG = LLM_CFGS["hd32"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def recs_of(rules_list):
    """aur_logit_rules records, one per dict (None = neutral)"""
    return np.concatenate([LR.records(LR.check_logit_rules(r), 1) for r in rules_list])


@pytest.fixture(scope="module")
def eng():
    e, _ = make_engine(CFG, 5, max_batch=8, max_new=24)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------------ 1 / 2. the kernels alone
@functools.lru_cache(maxsize=None)
def kernel_cases(vocab: int):
    """(rows fp32 [n, vocab], histories, records, eos, the definition's rows): computed once, shared by the apply and the restore
    test.  The host suite's cases at this vocabulary (short histories, every p x g x m), then the long ones: lengths around the
    workgroup's 1024 threads and up to 2047, one token 2047 times, ids 0 and vocab - 1, overlapping matches, the EOS in the history
    while n < m, neutral records, and neighbouring rows with different records over the same history."""
    rows, hist, recs = [], [], []
    if vocab <= 323:
        for _, row, h, rules, _ in cases((vocab,)):
            rows.append(row)
            hist.append(h)
            recs.append(dict(rules))
    rng = np.random.default_rng(vocab)
    base = make_row(vocab, 7)
    base[37] = np.nan                                                       # a NaN the history names: it stays a NaN
    pool = np.array([5, 11, 0, vocab - 1, 13, 17, 19, 23, 29, 31, 37, EOS, 41, 43])
    full = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=2048)
    for n in (0, 1, 2, 3, 1023, 1024, 1025, 2047):
        h = pool[rng.integers(0, len(pool), n)].tolist()                    # 14 tokens: every 2-gram and most 3-grams repeat
        for rules in (full, dict(repetition_penalty=0.8, no_repeat_ngram_size=2, min_new_tokens=n), dict(no_repeat_ngram_size=1),
                      dict(repetition_penalty=1.3), dict(min_new_tokens=n + 1), dict(repetition_penalty=1.0)):
            rows.append(base)
            hist.append(h)
            recs.append(rules)
    wide = rng.integers(0, vocab, 2047).tolist()                            # most of a small vocabulary, or 2047 different tokens
    for h in ([5] * 2047, [11] * 1025, ([5, 5, 5, EOS] * 512)[:2047], [0, vocab - 1] * 600, wide, wide[:1024] + wide[:1023]):
        for rules in (full, dict(repetition_penalty=0.8, no_repeat_ngram_size=4), dict(repetition_penalty=1.0)):
            rows.append(base)
            hist.append(h)
            recs.append(rules)
    want = np.stack([LR.apply(r, h, q, EOS) for r, h, q in zip(rows, hist, recs)])
    records = np.concatenate([LR.records(q, 1) for q in recs])
    return np.stack(rows), hist, records, recs, want


@pytest.mark.parametrize("vocab", [320, 323, 32000])
def test_kernel_alone_is_the_definition_bitwise(eng, vocab):
    rows, hist, records, recs, want = kernel_cases(vocab)
    got = eng.logit_rules_rows(torch.from_numpy(rows).cuda(), hist, records, EOS, restore=False, ids_stride=2048).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    bad = np.nonzero(((bits(got) != bits(want)) & ~np.isnan(want)).any(1))[0]
    assert len(bad) == 0, (len(bad), len(rows), [(int(i), len(hist[i]), recs[i]) for i in bad[:5]])
    assert np.array_equal(got, want, equal_nan=True)
    neutral = [i for i, q in enumerate(recs) if LR.check_logit_rules(q) is None]
    assert len(neutral) >= 8 and all(np.array_equal(bits(got[i]), bits(rows[i])) for i in neutral)      # bitwise untouched
    assert (bits(want) != bits(rows)).any(1).sum() > len(rows) // 4                                     # and many others are not
    # a history that fills the buffer exactly, and the engine's own stride (its longest history)
    full = [i for i, h in enumerate(hist) if len(h) == 2047][:4]
    tight = eng.logit_rules_rows(torch.from_numpy(rows[full]).cuda(), [hist[i] for i in full], records[full], EOS).cpu().numpy()
    assert np.array_equal(tight, want[full], equal_nan=True)
    no_eos = eng.logit_rules_rows(torch.from_numpy(rows[full]).cuda(), [hist[i] for i in full], records[full], None).cpu().numpy()
    assert np.array_equal(no_eos, np.stack([LR.apply(rows[i], hist[i], recs[i], None) for i in full]), equal_nan=True)


@pytest.mark.parametrize("vocab", [320, 323, 32000])
def test_restore_gives_every_row_back_bitwise(eng, vocab):
    rows, hist, records, _, _ = kernel_cases(vocab)
    got = eng.logit_rules_rows(torch.from_numpy(rows).cuda(), hist, records, EOS, restore=True, ids_stride=2048).cpu().numpy()
    assert np.array_equal(bits(got), bits(rows))


def test_kernel_clamps_what_the_host_would_reject(eng):
    """<= 0 / NaN penalties are 1, negative sizes are 0: such records are neutral, the row is not touched"""
    row = make_row(320, 3)
    recs = np.zeros(4, LR.RECORD)
    recs["repetition_penalty"] = [0.0, -2.0, np.nan, 1.0]
    recs["no_repeat_ngram"], recs["min_new_tokens"] = [0, -1, 0, -3], [0, -5, 0, 0]
    got = eng.logit_rules_rows(torch.from_numpy(np.stack([row] * 4)).cuda(), [[5, 5, 7, 11]] * 4, recs, EOS).cpu().numpy()
    assert all(np.array_equal(bits(g), bits(row)) for g in got)


# ------------------------------------------------------------------------------------------------------ 3 / 6. audit of the engine
def embeds(n, d, seed=0):
    return [torch.randn(40 + 7 * i, d, generator=torch.Generator().manual_seed(seed + i)).half().float() for i in range(n)]


def gen(e, emb, n_new=24, eos=None, **kw):
    return e.generate([padded(x) for x in emb], [x.shape[0] for x in emb], n_new, eos_id=eos, **kw)


SP = dict(temperature=0.9, top_k=40, top_p=0.9, seed=77)
AUDIT_RULES = [dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=6), dict(repetition_penalty=0.8, no_repeat_ngram_size=1),
               dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=3)]
REFILL_RULES = dict(no_repeat_ngram_size=1, min_new_tokens=4)
N_AUDIT = 16


@pytest.fixture(scope="module")
def audit():
    """Three slots with different records (0 and 1 greedy, 2 sampled), log-probabilities on, one step at a time with the engine's
    logits read after every step; then slot 1 is reset and re-filled with another record."""
    emb = embeds(3, CFG["hidden_size"], seed=2)
    e, _ = make_engine(CFG, 5, max_batch=3, max_new=N_AUDIT)
    try:
        eos = gen(e, emb, n_new=1)[0][0]                                     # what slot 0 would emit first: min_new_tokens has work to do
        e._rules_on()
        e._sampling_on()
        e._logprobs_on(2)
        e.begin_batch(3, N_AUDIT, eos)
        e.slot_logit_rules(0, recs_of(AUDIT_RULES))
        samp = S.records(S.check_sampling(SP), [0, 1, 9])
        samp[:2] = np.zeros(2, S.RECORD)                                     # slots 0 and 1: temperature 0 = greedy
        e.slot_sampling(0, samp)
        for b, x in enumerate(emb):
            e.prefill(b, padded(x), x.shape[0])
        logits = [e.logits().cpu().numpy()]
        for _ in range(N_AUDIT - 1):
            e.decode(1)
            logits.append(e.logits().cpu().numpy())
        out = e.outputs()
        lens, lp, tid, tlp = e.token_logprob_state()
        e.slot_reset(1)
        e.slot_logit_rules(1, recs_of([REFILL_RULES]))
        e.prefill(1, padded(emb[2]), emb[2].shape[0])
        again = [e.logits().cpu().numpy()[1]]
        for _ in range(5):
            e.decode(1)
            again.append(e.logits().cpu().numpy()[1])
        out2 = e.outputs()
        # the log-probability kernel alone on the raw rows the tokens were picked from
        rows = [(b, n) for b in range(3) for n in range(len(out[b]))]
        alone = e.token_logprob_rows(torch.from_numpy(np.stack([logits[n][b] for b, n in rows])).cuda(), [out[b][n] for b, n in rows], 2)
    finally:
        e.close()
    return dict(eos=eos, logits=logits, out=out, again=again, out2=out2, lp=(lens, lp, tid, tlp), rows=rows, alone=alone)


def assert_sampled_pick(row, tok, stream, n, tag):
    kept = int(S.kept_mask(row, SP["temperature"], SP["top_k"], SP["top_p"]).sum())
    idx, lo, hi = S.cdf_intervals(row, SP["temperature"], S.top_set(row, kept))
    j = np.nonzero(idx == tok)[0]
    assert len(j) == 1, tag
    u = S.uniform(SP["seed"], stream, n)
    observe("logit_rules/engine_draw_outside_f64_cdf_interval", max(lo[j[0]] - u, u - hi[j[0]], 0.0), EPS)


def test_every_emitted_token_is_the_pick_from_the_processed_row_of_the_gpus_own_logits(audit):
    eos, logits, out = audit["eos"], audit["logits"], audit["out"]
    assert all(np.isfinite(l).all() for l in logits) and all(np.isfinite(l).all() for l in audit["again"])      # the restore ran
    banned = 0
    for b in range(3):
        assert len(out[b]) >= 6 or out[b][-1] == eos
        for n in range(len(out[b])):
            row = LR.apply(logits[n][b], out[b][:n], AUDIT_RULES[b], eos)
            banned += int(np.isinf(row).any())
            if b < 2:
                assert out[b][n] == int(np.argmax(row)), (b, n)
            else:
                assert_sampled_pick(row, out[b][n], 9, n, (b, n))
    assert banned > 20
    assert len(out[0]) >= 6 and eos not in out[0][:5]                        # min_new_tokens held the EOS back on slot 0 ...
    assert int(np.argmax(logits[0][0])) == eos                               # ... which the raw row would have picked at once
    assert len(set(out[1])) == len(out[1])                                   # g = 1: no token twice
    # the re-filled slot: its own record, an empty history
    o2 = audit["out2"][1]
    assert len(o2) >= 4 and len(set(o2)) == len(o2)
    for n in range(len(o2)):
        assert o2[n] == int(np.argmax(LR.apply(audit["again"][n], o2[:n], REFILL_RULES, eos))), n
    assert audit["out2"][0] == out[0] and audit["out2"][2] == out[2]         # the neighbours went on undisturbed (finished: max_new)


def test_recorded_logprobs_are_those_of_the_unmodified_rows(audit):
    lens, lp, tid, tlp = audit["lp"]
    a_lp, a_tid, a_tlp = audit["alone"]
    assert [int(x) for x in lens] == [len(x) for x in audit["out"]]
    for k, (b, n) in enumerate(audit["rows"]):
        assert lp[b, n].tobytes() == a_lp[k].tobytes() and np.isfinite(lp[b, n]), (b, n)
        assert np.array_equal(tid[b, n], a_tid[k]) and tlp[b, n].tobytes() == a_tlp[k].tobytes(), (b, n)
        assert tid[b, n, 0] == int(np.argmax(audit["logits"][n][b]))         # rank 0 is the RAW row's maximum, banned or not


# ---------------------------------------------------------------------------------------------------------------- 4. the properties
def repeats(ids, g):
    grams = [tuple(ids[i:i + g]) for i in range(len(ids) - g + 1)]
    return len(grams) != len(set(grams))


@pytest.mark.parametrize("g", [2, 3])
def test_no_repeat_ngram_removes_the_loops_greedy_falls_into(eng, g):
    """hd32, weights seed 5: on the fp32 CPU model the greedy outputs of prompts 2, 5 and 7 fall into one loop (298 41 275 187 227
    132 1 108 ...) within 24 tokens.  The precondition is asserted on the GPU's own outputs."""
    emb = embeds(8, CFG["hidden_size"])
    plain = gen(eng, emb)
    looping = [b for b in range(8) if repeats(plain[b], g)]
    assert len(looping) >= 2, plain                                          # not vacuous
    ruled = gen(eng, emb, logit_rules=dict(no_repeat_ngram_size=g))
    assert all(len(x) == 24 and not repeats(x, g) for x in ruled), ruled
    for b in range(8):
        first = next((n for n in range(g, 25) if repeats(plain[b][:n], g)), 25)       # up to the first repeat nothing is banned
        assert ruled[b][:first - 1] == plain[b][:first - 1] and (b not in looping or ruled[b] != plain[b]), b


def test_min_new_tokens_holds_the_eos_back(eng):
    emb = embeds(4, CFG["hidden_size"])
    first = [x[0] for x in gen(eng, emb, n_new=1)]
    for b in (0, 3):
        eos = first[b]
        assert gen(eng, [emb[b]], eos=eos)[0] == [eos]                       # without the rule: length 1
        for m in (1, 7, 24):
            got = gen(eng, [emb[b]], eos=eos, logit_rules=dict(min_new_tokens=m))[0]
            assert len(got) >= m and eos not in got[:m] and (len(got) == 24 or got[-1] == eos), (b, m, got)


def test_neutral_rules_are_the_request_without_rules():
    emb = embeds(4, CFG["hidden_size"], seed=2)
    e, _ = make_engine(CFG, 5, max_batch=4)
    try:
        plain = gen(e, emb)
        neutral = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
        assert gen(e, emb, logit_rules=neutral) == plain and not e._rules_mode       # the option stays off
        assert gen(e, emb, logit_rules=dict(repetition_penalty=1.5)) != plain and e._rules_mode
        assert gen(e, emb, logit_rules=neutral) == plain and gen(e, emb) == plain    # the option on: neutral records
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 5. invariances
RULES = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=5)
OTHER = dict(repetition_penalty=0.7, no_repeat_ngram_size=1, min_new_tokens=20)


def mixed(e, emb, eos, recs, n_new=24):
    """one record per slot (None = a greedy neighbour without rules)"""
    e._rules_on()
    e.begin_batch(len(emb), n_new, eos)
    e.slot_logit_rules(0, recs_of(recs))
    for b, x in enumerate(emb):
        e.prefill(b, padded(x), x.shape[0])
    e.decode(n_new - 1)
    return e.outputs()


def test_ids_do_not_depend_on_batch_slot_neighbours_graph_or_bank():
    emb = embeds(8, CFG["hidden_size"])
    e, _ = make_engine(CFG, 5, max_batch=8)
    try:
        plain = gen(e, emb)
        eos = plain[2][0]                                                    # slot 2 would stop at once; 298 / 41 / ... loop on others
        a = gen(e, emb, eos=eos, logit_rules=RULES)
        assert a != gen(e, emb, eos=eos) and all(len(x) >= 5 for x in a)
        assert gen(e, emb, eos=eos, logit_rules=RULES) == a                  # the same call twice
        for b in (0, 2, 5):                                                  # alone in slot 0 == in the batch at slot b
            assert gen(e, [emb[b]], eos=eos, logit_rules=RULES)[0] == a[b]
        perm = [3, 0, 7, 1, 6, 2, 5, 4]                                      # another slot, other neighbours
        p = gen(e, [emb[i] for i in perm], eos=eos, logit_rules=RULES)
        assert [p[perm.index(i)] for i in range(8)] == a
        # neighbours with another record, and greedy neighbours without rules
        b_ = gen(e, emb, eos=eos, logit_rules=OTHER)
        g_ = gen(e, emb, eos=eos)
        m = mixed(e, emb, eos, [RULES, OTHER, None, RULES, None, OTHER, RULES, RULES])
        assert m == [a[0], b_[1], g_[2], a[3], g_[4], b_[5], a[6], a[7]]
    finally:
        e.close()
    e, _ = make_engine(CFG, 5, max_batch=8, use_graph=False)                 # eager launches
    try:
        assert gen(e, emb, eos=eos, logit_rules=RULES) == a
    finally:
        e.close()
    from aurora_amd.engine import AuroraCapEngine
    from tests.util import rand_llm_weights
    e = AuroraCapEngine({"vit": None, "llm": CFG}, {"llm": rand_llm_weights(CFG, 5)}, max_frames=1, max_batch=8, max_ctx=512,
                        max_new_tokens=24, num_banks=2)
    try:
        e.select_bank(1)
        assert gen(e, emb, eos=eos, logit_rules=RULES) == a
        e.select_bank(0)
        assert gen(e, emb, eos=eos, logit_rules=RULES) == a
    finally:
        e.close()


def test_caption_stream_slot_reuse_and_front_end_graphs_equal_each_clip_alone():
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_caption_batch import VCFG, weights
    N = 10
    gen_ = torch.Generator().manual_seed(21)
    clips = [(torch.randn(2 + i % 2, 3, 56, 56, generator=gen_).half().cuda(), [1, 20 + i] + [-200, 30 + i] * (2 + i % 2) + [40 + i] * (1 + i % 3))
             for i in range(7)]
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)
    e = AuroraCapEngine({"vit": VCFG, "llm": CFG}, weights(), max_frames=4, max_batch=3, max_ctx=512, max_new_tokens=N, spare_slots=2)
    try:
        free = [e.caption_ids(px, ids, 0.5, N, eos_id=None) for px, ids in clips]
        # the token that would cut the most clips short within three tokens: min_new_tokens has work, slots are freed at different times
        cands = sorted({t for x in free for t in x[:3]}, key=lambda t: (-sum(t in x[:3] for x in free), t))
        eos = cands[0]
        greedy = [e.caption_ids(px, ids, 0.5, N, eos_id=eos) for px, ids in clips]
        # the front-end graph case: clips without rules first (the graphs of their buckets are captured) ...
        got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=eos, check_every=4, overlap=True, front_graph=True))
        assert [got[i] for i in range(7)] == greedy and not e._rules_mode
        # ... then the same buckets with min_new_tokens alone, and with all three rules
        for r in (dict(min_new_tokens=4), rules):
            alone = [e.caption_ids(px, ids, 0.5, N, eos_id=eos, logit_rules=r) for px, ids in clips]
            assert alone != greedy and all(len(x) >= r["min_new_tokens"] for x in alone)
            assert e.caption_batch(clips[:3], 0.5, N, eos_id=eos, logit_rules=r) == alone[:3]
            for kw in (dict(overlap=True, front_graph=True), dict(overlap=True, front_graph=False), dict(overlap=False)):
                for check_every in (4, 2):
                    got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=eos, check_every=check_every, logit_rules=r, **kw))
                    assert [got[i] for i in range(7)] == alone, (r, kw, check_every)
        got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=eos, check_every=4, overlap=True))          # no rules again, same ctx
        assert [got[i] for i in range(7)] == greedy
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------ 7. the public ways in
def test_llm_generate_and_caption_batch_on_the_checkpoint_fixture(tmp_path):
    from tests.test_gpu_sampling import _ckpt_model
    g = golden("g13_checkpoint_e2e.npz")
    m, _ = _ckpt_model(tmp_path)
    try:
        m.visual_encoder.reset_tome_r(float(g["ratio"]))
        px = torch.from_numpy(g["pixel_values"]).cuda()
        data = {"pixel_values": px.unsqueeze(0), "input_ids": torch.from_numpy(g["input_ids"])}

        def run(**kw):
            return m.llm.generate(**m(data, mode="inference"), num_beams=1, max_new_tokens=12, eos_token_id=None, **kw)[0].tolist()
        plain = run()
        assert run(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0) == plain
        a = run(repetition_penalty=1.3, no_repeat_ngram_size=1)
        assert len(a) == 12 and len(set(a)) == 12 and a[0] == plain[0]
        assert a == run(repetition_penalty=1.3, no_repeat_ngram_size=1)
        ids = g["input_ids"][0].tolist()
        assert m.caption_batch([(px, ids)], max_new_tokens=12, eos_token_id=None,
                               logit_rules=dict(repetition_penalty=1.3, no_repeat_ngram_size=1)) == [a]
        eos = plain[0]
        short = m.llm.generate(**m(data, mode="inference"), max_new_tokens=12, eos_token_id=eos)[0].tolist()
        held = m.llm.generate(**m(data, mode="inference"), max_new_tokens=12, eos_token_id=eos, min_new_tokens=5)[0].tolist()
        assert short == [eos] and len(held) >= 5 and eos not in held[:5]
        with pytest.raises(ValueError):
            run(repetition_penalty=0.0)
        m.llm.generation_logit_rules = dict(no_repeat_ngram_size=1, repetition_penalty=1.3)          # as generation_config.json sets them
        assert run() == a and run(no_repeat_ngram_size=0, repetition_penalty=1.0) == plain
    finally:
        m.engine.close()


def test_plugin_gen_kwargs_on_the_real_engine(tmp_path):
    """Four requests about the same clip with the same prompt, so that all of them have the same greedy caption P; with the EOS set
    to P[0] a request without rules ends after one token, and one with min_new_tokens goes on."""
    from types import SimpleNamespace
    from transformers import AutoTokenizer
    from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
    from tests.test_gpu_sampling import _ckpt_model
    m, src = _ckpt_model(tmp_path, max_batch=2)
    try:
        tok = AutoTokenizer.from_pretrained(src, padding_side="right")

        def pre(frames):                                                  # frames [f, H, W, 3] uint8 -> [f, 3, 56, 56] fp16
            x = frames.permute(0, 3, 1, 2).float() / 255.0
            return torch.nn.functional.interpolate(x, size=(56, 56), mode="bilinear").half()
        frames = np.random.default_rng(3).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
        docs = {i: frames for i in range(4)}
        ruled = {"max_new_tokens": 8, "min_new_tokens": 4, "no_repeat_ngram_size": 1, "repetition_penalty": 1.3}
        gens = [ruled, {"max_new_tokens": 8}, ruled, {"max_new_tokens": 8}]
        reqs = [SimpleNamespace(args=("describe it", gens[i], lambda d: [d], i, "t", "s")) for i in range(4)]
        captured = []
        deliver = m.caption_stream

        def spy(*a, **kw):                                                # the ids behind the decoded text
            for k, ids in deliver(*a, **kw):
                captured.append((kw.get("logit_rules"), list(ids)))
                yield k, ids
        m.caption_stream = spy

        def plugin():
            p = P.AuroraCapMI355X(pretrained="unused", device="cuda", batch_size=2, _model=m, _tokenizer=tok, _preprocessor=pre)
            p.task_dict = {"t": {"s": docs}}
            return p
        m.llm.eos_token_id = None
        plugin().generate_until([SimpleNamespace(args=(r.args[0], {"max_new_tokens": 8}) + r.args[2:]) for r in reqs])
        caption = captured[0][1]
        assert len(captured) == 4 and all(r is None and ids == caption for r, ids in captured) and len(caption) == 8
        m.llm.eos_token_id = caption[0]
        captured.clear()
        texts = plugin().generate_until(reqs)
        assert len(texts) == 4 and len(captured) == 4 and texts[0] == texts[2] and texts[1] == texts[3] and texts[0] != texts[1]
        with_rules = [ids for r, ids in captured if r]
        without = [ids for r, ids in captured if not r]
        assert without == [[caption[0]]] * 2                                                          # the EOS at once
        assert len(with_rules) == 2 and with_rules[0] == with_rules[1]
        assert len(with_rules[0]) >= 4 and caption[0] not in with_rules[0][:4] and len(set(with_rules[0])) == len(with_rules[0])
        assert all(r == dict(repetition_penalty=float(np.float32(1.3)), no_repeat_ngram_size=1, min_new_tokens=4) for r, _ in captured if r)
        with pytest.raises(ValueError):
            plugin().generate_until([SimpleNamespace(args=("x", {"repetition_penalty": "1.3"}, lambda d: [d], 0, "t", "s"))])
    finally:
        m.engine.close()


def test_cli_no_repeat_ngram_size():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--synthetic", "--no_repeat_ngram_size", "3",
                          "--repetition_penalty", "1.2", "--min_new_tokens", "4", "--max_new_tokens", "12"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    ids = [int(x) for x in out.stdout.strip().split("\n")[-1].strip("[]").split(",")]           # --synthetic prints the ids
    assert len(ids) == 12 and not repeats(ids, 3)

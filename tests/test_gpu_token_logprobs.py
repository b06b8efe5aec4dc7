"""GPU: log-probabilities of GENERATED tokens on the path (`logprobs=` of generate / caption_ids / caption_batch / caption_prompts /
caption_stream, the `_LLM.generate` seam, `inference.py --logprobs`).

The record of a token is bitwise what aur_score_rows / aur_token_logprob_rows say about the logits row it was picked from - the kernel
behind the pick and the stand-alone kernels are one evaluation (tests/test_gpu_logprob_rows.py holds that evaluation to the float64
definition) - so every comparison here is on bytes, except the one against `loglikelihood_batch`, whose logits come from other kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.parity_bounds import LOGIT_TOL
from tests.test_gpu_llm import LLM_CFGS, make_engine, padded
from tests.util import rand_llm_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS, NEW = (40, 97, 33), 12
SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)


def prompts(cfg, lens=LENS, seed=21):
    gen = torch.Generator().manual_seed(seed)
    return [padded(torch.randn(L, cfg["hidden_size"], generator=gen).half().float()) for L in lens]


def same(a, b):
    """two result dicts: the same ids and the same bytes"""
    return a["ids"] == b["ids"] and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
                                        for k in ("token_logprobs", "top_ids", "top_logprobs"))


def cut(r, n):
    return dict(ids=r["ids"][:n], token_logprobs=r["token_logprobs"][:n], top_ids=r["top_ids"][:n], top_logprobs=r["top_logprobs"][:n])


def check_shapes(r, n_top, vocab):
    n = len(r["ids"])
    assert r["token_logprobs"].dtype == np.float32 and r["token_logprobs"].shape == (n,)
    assert r["top_ids"].dtype == np.int32 and r["top_ids"].shape == (n, n_top)
    assert r["top_logprobs"].dtype == np.float32 and r["top_logprobs"].shape == (n, n_top)
    assert (r["token_logprobs"] <= 0).all() and (r["top_ids"] >= 0).all() and (r["top_ids"] < vocab).all()
    if n_top:
        assert (np.diff(r["top_logprobs"], axis=1) <= 0).all() and (r["token_logprobs"] <= r["top_logprobs"][:, 0]).all()


@pytest.fixture(scope="module")
def eng3():
    """hd32, three slots, captured decode step; `embs()` gives the three prompts, `plain` their ids BEFORE anything asked for
    log-probabilities"""
    cfg = LLM_CFGS["hd32"]
    e, _ = make_engine(cfg, 5, max_batch=3, use_graph=True, max_new=NEW)
    base = prompts(cfg)

    def embs():                                                   # a prefill clobbers its embeddings: fresh copies for every use
        return [x.clone() for x in base]
    plain = {None: e.generate(embs(), LENS, NEW, eos_id=None), "sampled": e.generate(embs(), LENS, NEW, eos_id=None, sampling=SAMPLED)}
    assert not e._lp_top and not e._lp_bufs                          # a process that never asks allocates nothing
    yield e, cfg, embs, plain
    e.close()


def test_the_ids_do_not_change_greedy_or_sampled(eng3):
    eng, cfg, embs, plain = eng3
    for n in (0, 3, 8):
        got = eng.generate(embs(), LENS, NEW, eos_id=None, logprobs=n)
        assert [r["ids"] for r in got] == plain[None]
        smp = eng.generate(embs(), LENS, NEW, eos_id=None, sampling=SAMPLED, logprobs=n)
        assert [r["ids"] for r in smp] == plain["sampled"]
        for r in got + smp:
            check_shapes(r, n, cfg["vocab_size"])
        for r in got:                                                 # greedy: the picked token is rank 0, with its bits
            if n:
                assert r["top_ids"][:, 0].tolist() == r["ids"] and r["top_logprobs"][:, 0].tobytes() == r["token_logprobs"].tobytes()
    assert plain[None] != plain["sampled"]
    assert eng.generate(embs(), LENS, NEW, eos_id=None) == plain[None]              # still recording (sticky); the plain return value


def stepwise(eng, first_tokens, nnew, top, eos=None, extra_steps=0):
    """first_tokens(): the prefills / commits; then decode(1) at a time.  After every step each slot that appended a token is checked
    against the stand-alone kernels on a copy of its logits row.  Returns (final state, ids)."""
    B = eng._batch
    seen = [0] * B
    checked = 0
    for step in range(nnew + extra_steps):
        if step == 0:
            first_tokens()
        else:
            eng.decode(1)
        logits, ids = eng.logits(), eng.outputs()
        lens, lp, tid, tlp = eng.token_logprob_state()
        assert lens.tolist() == [len(x) for x in ids]
        for b in range(B):
            n = len(ids[b])
            if n == seen[b]:
                continue                                              # finished or idle: nothing appended, nothing recorded
            assert n == seen[b] + 1
            seen[b] = n
            row, tok = logits[b:b + 1].contiguous(), [ids[b][-1]]
            s_lp, _ = eng.score_rows(row, tok)
            r_lp, r_ids, r_lps = eng.token_logprob_rows(row, tok, top)
            assert lp[b, n - 1].tobytes() == s_lp[0].tobytes() == r_lp[0].tobytes(), (step, b)
            assert tid[b, n - 1, :top].tobytes() == r_ids[0].tobytes() and tlp[b, n - 1, :top].tobytes() == r_lps[0].tobytes(), (step, b)
            checked += 1
        for b in range(B):                                            # beyond every slot's length: 0 / (-1, 0)
            assert (lp[b, seen[b]:] == 0).all() and (tid[b, seen[b]:] == -1).all() and (tlp[b, seen[b]:] == 0).all()
    return (lens, lp, tid, tlp), ids, checked


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_every_step_records_what_the_row_kernels_say(eng3, mode):
    eng, cfg, embs, plain = eng3
    from aurora_amd import sampling as S
    eng._logprobs_on(3)
    if mode == "sampled":
        eng._sampling_on()
    eng.begin_batch(3, NEW, None)
    if mode == "sampled":
        eng.slot_sampling(0, S.records(S.check_sampling(SAMPLED), [0, 1, 2]))

    fresh = embs()                                                # alive until the steps behind the prefills have synchronised

    def first():
        for b in range(3):
            eng.prefill(b, fresh[b], LENS[b])
    _, ids, checked = stepwise(eng, first, NEW, 3)
    assert checked == 3 * NEW and ids == plain[None if mode == "greedy" else "sampled"]


def test_first_tokens_from_a_commit_at_slot0_above_0():
    """slot 0 prefilled in place, slots 1 and 2 staged into spare sequences and committed together: the commit clears and records
    slots [1, 3) only"""
    from aurora_amd.engine import AuroraCapEngine
    cfg = LLM_CFGS["hd32"]
    eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 5)}, max_frames=1, max_batch=3, max_ctx=512,
                          max_new_tokens=NEW, spare_slots=2)
    try:
        gen = torch.Generator().manual_seed(33)
        e0 = padded(torch.randn(40, cfg["hidden_size"], generator=gen).half().float())
        pair = torch.cat([padded(torch.randn(70, cfg["hidden_size"], generator=gen).half().float()) for _ in range(2)], 0)
        keep = pair.clone()
        eng._logprobs_on(2)
        eng.begin_batch(3, NEW, None)
        eng.slot_retire(1)
        eng.slot_retire(2)

        def first():
            eng.prefill(0, e0, 40)
            eng.prefill_stage(3, 2, pair, 70)
            eng.prefill_commit(1, 2, 3, pair, 70)
        state, ids, checked = stepwise(eng, first, NEW, 2)
        assert checked == 3 * NEW and [len(x) for x in ids] == [NEW] * 3
        alone = eng.generate([keep[:96].clone()], [70], NEW, eos_id=None, logprobs=2)[0]
        assert alone["ids"] == ids[1] and alone["token_logprobs"].tobytes() == state[1][1].tobytes()
        assert alone["top_ids"].tobytes() == state[2][1].tobytes()
    finally:
        eng.close()


def test_stopping_at_eos_and_at_max_new(eng3):
    eng, cfg, embs, plain = eng3
    free = eng.generate(embs(), LENS, NEW, eos_id=None, logprobs=3)
    # an id of slot 1's first tokens that some other slot never emits: slot 1 stops early, that slot fills max_new
    eos = next(t for t in free[1]["ids"][:NEW - 2] if any(t not in r["ids"] for r in free))
    stop = [r["ids"].index(eos) + 1 if eos in r["ids"] else NEW for r in free]
    assert stop[1] < NEW - 1 and max(stop) == NEW, stop
    eng._logprobs_on(3)
    eng.begin_batch(3, NEW, eos)

    fresh = embs()                                                # alive until the steps behind the prefills have synchronised

    def first():
        for b in range(3):
            eng.prefill(b, fresh[b], LENS[b])
    (lens, lp, tid, tlp), ids, checked = stepwise(eng, first, NEW, 3, eos=eos, extra_steps=4)     # steps past the end record nothing
    assert lens.tolist() == stop and checked == sum(stop)
    for b in range(3):                                                # up to the stop: the bits of the run without that EOS
        got = dict(ids=ids[b], token_logprobs=lp[b, :stop[b]], top_ids=tid[b, :stop[b], :3], top_logprobs=tlp[b, :stop[b], :3])
        assert same(got, cut(free[b], stop[b])), b
    assert [same(r, cut(f, s)) for r, f, s in zip(eng.generate(embs(), LENS, NEW, eos_id=eos, check_every=4, logprobs=3), free, stop)] == [True] * 3


def test_captured_and_eager_steps_give_the_same_bits():
    """the two launch forms of test_greedy_matches_oracle_ids_and_graph_equals_eager, hd128"""
    cfg = LLM_CFGS["hd128"]
    emb = torch.randn(50, cfg["hidden_size"], generator=torch.Generator().manual_seed(3)).half().float()
    outs = []
    for use_graph in (False, True):
        eng, _ = make_engine(cfg, 6, max_batch=1, use_graph=use_graph)
        try:
            plain = eng.generate([padded(emb)], [50], 20, eos_id=None)[0]
            outs.append(eng.generate([padded(emb)], [50], 20, eos_id=None, logprobs=2)[0])
            assert outs[-1]["ids"] == plain and len(plain) == 20
            check_shapes(outs[-1], 2, cfg["vocab_size"])
        finally:
            eng.close()
    assert same(outs[0], outs[1])


def test_off_after_on_leaves_the_buffer_alone(eng3):
    eng, cfg, embs, plain = eng3
    on = eng.generate(embs(), LENS, NEW, eos_id=None, logprobs=8)
    buf = eng._lp_bufs[eng._bank]
    eng.logprobs_off()
    assert not eng._lp_top
    torch.cuda.synchronize()
    buf.fill_(0xA5)
    assert eng.generate(embs(), LENS, NEW, eos_id=None) == plain[None] == [r["ids"] for r in on]
    eng.begin_batch(3, NEW, None)                                     # the calls that clear records when it is on
    eng.slot_reset(1)
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), "a bank that no longer records wrote its old buffer"
    with pytest.raises(Exception):
        eng.token_logprob_state()
    assert [same(a, b) for a, b in zip(eng.generate(embs(), LENS, NEW, eos_id=None, logprobs=8), on)] == [True] * 3      # and on again


def test_a_sequence_in_a_batch_of_3_gets_what_it_gets_alone(eng3):
    eng, cfg, embs, plain = eng3
    for samp in (None, SAMPLED):
        kw = dict(sampling=samp) if samp else {}
        together = eng.generate(embs(), LENS, NEW, eos_id=None, logprobs=4, **kw)
        for b in range(3):
            alone = eng.generate([embs()[b]], [LENS[b]], NEW, eos_id=None, logprobs=4, **(dict(kw, streams=[b]) if samp else {}))[0]
            assert same(alone, together[b]), (b, samp is not None)


def test_slot_collect_logprobs_copies_the_records_on_the_device(eng3):
    eng, cfg, embs, plain = eng3
    got = eng.generate(embs(), LENS, NEW, eos_id=None, logprobs=2)
    top = eng._lp_top[eng._bank]
    lp = torch.empty(2, NEW, dtype=torch.float32, device="cuda")
    tid = torch.empty(2, NEW, top, dtype=torch.int32, device="cuda")
    tlp = torch.empty(2, NEW, top, dtype=torch.float32, device="cuda")
    lens = torch.empty(2, dtype=torch.int32, device="cuda")
    eng.slot_collect_logprobs(1, 2, lp, tid, tlp, lens)
    torch.cuda.synchronize()
    assert lens.tolist() == [NEW, NEW]
    for j in range(2):
        assert lp[j].cpu().numpy().tobytes() == got[1 + j]["token_logprobs"].tobytes()
        assert tid[j, :, :2].cpu().numpy().tobytes() == got[1 + j]["top_ids"].tobytes()
        assert tlp[j, :, :2].cpu().numpy().tobytes() == got[1 + j]["top_logprobs"].tobytes()


# ------------------------------------------------------------------------------------------------ the whole path (tiny ViT + projector + Llama)
def whole_path_engine(max_batch, max_new, spare=0, max_frames=4):
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_caption_batch import VCFG, weights
    return AuroraCapEngine({"vit": VCFG, "llm": LLM_CFGS["hd32"]}, weights(), max_frames=max_frames, max_batch=max_batch, max_ctx=512,
                           max_new_tokens=max_new, spare_slots=spare)


@pytest.mark.parametrize("spare", [0, 2])
def test_continuous_batching_gives_every_clip_what_it_gets_alone(spare):
    """7 ragged clips through 3 slots with EOS stopping, so that slots are refilled: spare = 0 is the plain schedule (overlap=False),
    spare = 2 the overlapped one (front ends staged beside the decode, committed into freed slots)"""
    from tests.test_gpu_caption_batch import clips
    eng = whole_path_engine(3, NEW, spare)
    try:
        cs = clips(7, 9)
        free = [eng.caption_ids(px, ids, 0.5, NEW, eos_id=None) for px, ids in cs]
        eos = free[2][5]
        want = [eng.caption_ids(px, ids, 0.5, NEW, eos_id=eos, logprobs=2) for px, ids in cs]
        assert [w["ids"] for w in want] == [a[: a.index(eos) + 1] if eos in a else a for a in free]
        assert len({len(w["ids"]) for w in want}) > 1
        got = dict(eng.caption_stream(cs, 0.5, NEW, eos_id=eos, check_every=4, logprobs=2, **({} if spare else dict(overlap=False))))
        assert sorted(got) == list(range(7))
        for i in range(7):
            check_shapes(got[i], 2, LLM_CFGS["hd32"]["vocab_size"])
            assert same(got[i], want[i]), i
    finally:
        eng.close()


def test_shared_prefix_and_unshared_front_ends_record_the_same():
    from tests.test_gpu_shared_prefix import FRAMES, RATIO, TAILS
    eng = whole_path_engine(3, NEW, max_frames=FRAMES)
    try:
        px = torch.randn(FRAMES, 3, 56, 56, generator=torch.Generator().manual_seed(90)).half().cuda()
        ps = [[1] + [-200, 30] * FRAMES + TAILS[p] for p in "ABC"]
        shared = eng.caption_prompts(px, ps, RATIO, NEW, eos_id=None, logprobs=3)
        plain = eng.caption_batch([(px, p) for p in ps], RATIO, NEW, eos_id=None, logprobs=3)
        assert [same(a, b) for a, b in zip(shared, plain)] == [True] * 3
        assert same(shared[1], eng.caption_ids(px, ps[1], RATIO, NEW, eos_id=None, logprobs=3))
    finally:
        eng.close()


def test_against_scoring_the_same_caption_on_the_prefill_path():
    """Per token |recorded lp - loglikelihood_batch's lp| <= 4 * LOGIT_TOL * max|logit| of that token's row: each path's logits are
    within LOGIT_TOL * max|logit| of the oracle's (tests/test_gpu_llm.py, tests/test_gpu_score.py), so the two rows are within twice
    that of each other, and lp - a logit minus a log-sum-exp of the row - is 2-Lipschitz in the sup norm of its row."""
    from tests.test_gpu_loglikelihood import IDS
    eng = whole_path_engine(3, 8, max_frames=3)
    try:
        px = torch.randn(3, 3, 56, 56, generator=torch.Generator().manual_seed(76)).half().float()
        vis = eng.vit_encode(px, eng.tome_r(0.5))
        emb, L = eng.project_splice(vis, IDS)
        eng._logprobs_on(0)
        eng.begin_batch(1, 8, None)
        eng.prefill(0, emb, L)
        scale = [eng.logits()[0].abs().max().item()]
        for _ in range(7):
            eng.decode(1)
            scale.append(eng.logits()[0].abs().max().item())
        rec = eng.outputs(logprobs=0)[0]
        assert len(rec["ids"]) == 8
        r = eng.loglikelihood_batch([(px, IDS, rec["ids"])], 0.5)[0]
        for j in range(8):
            err, bound = abs(float(rec["token_logprobs"][j]) - r["token_logprobs"][j]), 4 * LOGIT_TOL * scale[j]
            print(f"token {j}: |generated lp - scored lp| = {err:.3e} = {err / bound:.4f} of the bound {bound:.3e}")
            assert err <= bound, j
    finally:
        eng.close()


def test_the_generate_seam_returns_an_object_with_tensors():
    from aurora_amd.model import AuroraModel, GenerateOutput
    from tests.test_gpu_loglikelihood import IDS
    eng = whole_path_engine(1, 8, max_frames=3)
    try:
        m = AuroraModel(eng, eos_token_id=None)
        m.visual_encoder.reset_tome_r(0.5)
        px = torch.randn(3, 3, 56, 56, generator=torch.Generator().manual_seed(76)).half()
        out = m({"pixel_values": px.unsqueeze(0), "input_ids": torch.tensor([IDS])}, mode="inference")
        plain = m.llm.generate(**out, do_sample=False, max_new_tokens=8)
        assert torch.is_tensor(plain) and plain.shape == (1, 8)
        r = m.llm.generate(**out, do_sample=False, max_new_tokens=8, return_dict_in_generate=True, output_logprobs=True, top_logprobs=2,
                           output_scores=True)
        assert isinstance(r, GenerateOutput) and torch.equal(r.sequences, plain) and r.sequences.dtype == torch.long
        assert r.token_logprobs.shape == (1, 8) and r.token_logprobs.dtype == torch.float32
        assert r.top_ids.shape == (1, 8, 2) and r.top_logprobs.shape == (1, 8, 2) and r.top_logprobs.dtype == torch.float32
        assert torch.equal(r.top_ids[0, :, 0], plain[0]) and torch.equal(r.top_logprobs[0, :, 0], r.token_logprobs[0])
        bare = m.llm.generate(**out, do_sample=False, max_new_tokens=8, return_dict_in_generate=True)
        assert torch.equal(bare.sequences, plain) and bare.token_logprobs is None
        with pytest.raises(ValueError):
            m.llm.generate(**out, max_new_tokens=8, output_logprobs=True)
        got = m.caption_batch([(px, IDS)], max_new_tokens=8, logprobs=2)[0]
        assert got["ids"] == plain[0].tolist() and got["token_logprobs"].tobytes() == r.token_logprobs[0].numpy().tobytes()
    finally:
        eng.close()


def test_cli_prints_one_line_per_token_and_their_sum():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--synthetic", "--logprobs", "2", "--max_new_tokens", "8"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().split("\n")
    ids = [int(x) for x in lines[-10].strip("[]").split(",")]          # --synthetic prints the ids
    assert len(ids) == 8
    total = 0.0
    for i, line in enumerate(lines[-9:-1]):
        f = line.split()
        assert f[0] == "token" and int(f[1]) == i and f[2] == "id" and int(f[3]) == ids[i] and f[5] == "logprob" and f[7] == "top", line
        lp = float(f[6])
        alts = [(int(a.split(":")[0]), float(a.split(":")[1])) for a in f[8:]]
        assert len(alts) == 2 and alts[0] == (ids[i], lp) and alts[1][1] <= lp <= 0, line          # greedy: the pick is rank 0
        total += lp
    f = lines[-1].split()
    assert f[0] == "sum_logprob" and f[2] == "perplexity"
    assert float(f[1]) == total and abs(float(f[3]) - np.exp(-total / 8)) <= 1e-9 * np.exp(-total / 8)

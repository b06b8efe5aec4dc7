"""Stop token ids, stop strings and per-request budgets on the GPU.
  1. the kernel alone (aur_stop_rows) is `aurora_amd.stopping`, exactly;  2. the engine stops where the definition cuts the free run;
  3. the ids do not depend on batch, slot, bank, graph, slot reuse or a commit's pick;  4. unasked means unchanged;
  5. log-probabilities and logit rules beside a stop;  6. llm.generate, the lmms-eval adaptor and the CLI.
The definition itself is checked against transformers in tests/test_stopping_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from aurora_amd import stopping as ST
from tests import stopping_cases as SC
from tests.test_gpu_llm import LLM_CFGS, make_engine, padded
from tests.util import golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = LLM_CFGS["hd32"]
NEW = 24
SP = dict(temperature=0.9, top_k=40, top_p=0.9, seed=77)


@functools.lru_cache(maxsize=None)
def small_table(vocab: int = 320):
    """2 to 6 lower-case letters per token: what the tiny engines' ids decode to in these tests"""
    rng = np.random.default_rng(11)
    return ST.table_from_list([bytes(rng.integers(97, 123, int(rng.integers(2, 7))).astype(np.uint8)) for _ in range(vocab)])


TAB = small_table()


@pytest.fixture(scope="module")
def eng():
    e, _ = make_engine(CFG, 5, max_batch=8, max_new=NEW)
    e.set_stop_vocab(TAB)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------------ 1. the kernel alone
def want_flags(hist, recs, table, bmax, before):
    out = np.array(before, np.int32)
    for i, (h, r) in enumerate(zip(hist, recs)):
        if before[i] == 0 and len(h) >= 1 and ST.fires(h, ST.from_record(r), table, None, bmax) is not None:
            out[i] = 1
    return out


def run_rows(eng, hist, recs, table, bmax, stride=None):
    """every row once with its flag clear and once among rows whose flag is already set (7: it must come back as it was)"""
    recs = np.array(recs, ST.RECORD)
    clear = np.zeros(len(hist), np.int32)
    got = eng.stop_rows(hist, recs, bmax, table=table, ids_stride=stride)
    want = want_flags(hist, recs, table, bmax, clear)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), len(hist), [(int(i), hist[i], ST.from_record(recs[i]), int(got[i]), int(want[i])) for i in bad[:4]])
    mixed = np.where(np.arange(len(hist)) % 3 == 1, 7, 0).astype(np.int32)
    got2 = eng.stop_rows(hist, recs, bmax, finished=mixed, table=table, ids_stride=stride)
    assert np.array_equal(got2, want_flags(hist, recs, table, bmax, mixed))
    return want


def test_kernel_alone_on_the_host_suites_cases(eng):
    from transformers import AutoTokenizer
    table = ST.token_bytes(AutoTokenizer.from_pretrained(SC.TINY))
    seqs = SC.seeded_sequences()
    rec = ST.records([ST.check_stop(dict(strings=SC.STRINGS), None, table)])[0]
    want = run_rows(eng, seqs, [rec] * len(seqs), table, 64)
    assert int(want.sum()) == 262                                             # what StopStringCriteria says of these sequences
    dt, _ = SC.doc_table()
    cases = SC.doc_cases()
    rec = ST.records([ST.check_stop(dict(strings="stop"), None, dt)])[0]
    want = run_rows(eng, [h for h, _ in cases], [rec] * len(cases), dt, 64)
    assert want.tolist() == [int(f) for _, f in cases]


def test_kernel_alone_on_a_32000_entry_table(eng):
    """histories of 1 to 40 tokens of 0 to 255 bytes; strings cut out of the history's own text (so that most of them occur
    somewhere, some of them at the end), random ones, stop ids from the history, budgets around its length"""
    table = SC.synthetic_table()
    V = len(table[0]) - 1
    rng = np.random.default_rng(3)
    special = [0, 9, 7, 1000, V - 1]                                          # the tokens of 0 and of 255 bytes
    hist, recs = [], []
    for i in range(1500):
        n = int(rng.integers(1, 41))
        h = rng.integers(0, V, n).tolist()
        for _ in range(int(rng.integers(0, 3))):
            h[int(rng.integers(0, n))] = special[int(rng.integers(0, len(special)))]
        text = b"".join(ST.bytes_of(table, t) for t in h)
        strings = []
        for _ in range(int(rng.integers(0, 9))):
            L = int(rng.integers(1, 65))
            if len(text) >= L and rng.random() < 0.8:
                e = len(text) - int(rng.integers(0, 12)) if rng.random() < 0.7 else int(rng.integers(L, len(text) + 1))
                e = max(e, L)
                strings.append(text[e - L:e])
            else:
                strings.append(bytes(rng.integers(97, 101, L).astype(np.uint8)))
        ids = [h[int(rng.integers(0, n))] for _ in range(int(rng.integers(0, 3)))] if rng.random() < 0.3 else []
        budget = int(rng.integers(max(1, n - 1), n + 3)) if rng.random() < 0.2 else 0
        hist.append(h)
        recs.append(ST.records([dict(token_ids=ids, strings=strings, max_new_tokens=min(budget, 64))])[0])
    want = run_rows(eng, hist, recs, table, 64, stride=40)
    assert 300 < int(want.sum()) < 1200, int(want.sum())                      # neither answer passes by default
    reasons = {ST.fires(h, ST.from_record(r), table, None, 64)[0] for h, r, w in zip(hist, recs, want) if w}
    assert reasons == {"stop_token", "stop_string", "length"}


def test_kernel_alone_at_the_edges(eng):
    rows = SC.edge_rows()
    fired = 0
    for bmax in sorted({r[2] for r in rows}):
        grp = [r for r in rows if r[2] == bmax]
        want = run_rows(eng, [r[0] for r in grp], [r[1] for r in grp], SC.edge_table(), bmax)
        fired += int(want.sum())
        assert all(w == 0 for r, w in zip(grp, want) if len(r[0]) == 0)       # n = 0
    assert 15 <= fired <= len(rows) - 12
    # without a byte table no string matches; ids and budgets still do
    grp = [r for r in rows if r[2] == 64 and len(r[0])]
    got = eng.stop_rows([r[0] for r in grp], np.array([r[1] for r in grp], ST.RECORD), 64)
    want = [int(ST.fires(r[0], ST.from_record(r[1]), None, None, 64) is not None) for r in grp]
    assert got.tolist() == want and 0 < sum(want) < len(want)


# ------------------------------------------------------------------------------------------- 2. the engine and the definition
def embeds(n, d, seed=0):
    return [torch.randn(40 + 7 * i, d, generator=torch.Generator().manual_seed(seed + i)).half().float() for i in range(n)]


def gen(e, emb, n_new=NEW, eos=None, **kw):
    return e.generate([padded(x) for x in emb], [x.shape[0] for x in emb], n_new, eos_id=eos, **kw)


def tb(t):
    return ST.bytes_of(TAB, int(t))


def derived(free):
    """eight different records from the free run's ids, one per slot"""
    return [None,
            dict(token_ids=[free[1][3]]),
            dict(token_ids=[free[2][0]]),                                     # fires on the prefill's pick
            dict(strings=[tb(free[3][4]) + tb(free[3][5])]),
            dict(strings=[tb(free[4][5]) + tb(free[4][6])[:1]]),              # ends inside token 6 (every token has 2 bytes or more)
            dict(max_new_tokens=1),
            dict(max_new_tokens=5),
            dict(strings=["ZZ"], token_ids=[319 if 319 not in free[7] else 318])]


def cut(ids, stop, eos=None, n_new=NEW):
    rec = ST.check_stop(stop, n_new, TAB)
    n = ST.first_stop(ids, rec, TAB, eos, n_new)
    return list(ids) if n is None else list(ids[:n])


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_engine_stops_where_the_definition_cuts_the_free_run(eng, sampled):
    emb = embeds(8, CFG["hidden_size"])
    kw = dict(sampling=SP) if sampled else {}
    free = gen(eng, emb, **kw)
    assert all(len(x) == NEW for x in free)
    stops = derived(free)
    got = gen(eng, emb, stop=stops, **kw)
    want = [cut(free[b], stops[b]) for b in range(8)]
    assert got == want, (got, want)
    reasons = [ST.finish_reason(got[b], ST.check_stop(stops[b], NEW, TAB), TAB, None, NEW) for b in range(8)]
    assert [r[0] for r in reasons[:3]] == ["length", "stop_token", "stop_token"] and len(got[2]) == 1 and len(got[1]) <= 4
    assert reasons[3] == ("stop_string", 0) and reasons[4] == ("stop_string", 0) and len(got[3]) <= 6 and len(got[4]) <= 7
    assert reasons[5] == ("length", None) and len(got[5]) == 1 and reasons[6][0] in ("length", "stop_token", "stop_string") and len(got[6]) <= 5
    assert got[0] == free[0] and got[7] == free[7] and reasons[7] == ("length", None)
    assert sum(len(x) < NEW for x in got) == 6
    # the batch's EOS comes first when both hold, and stops a slot that has no record
    eos = free[1][3]
    got = gen(eng, emb, eos=eos, stop=stops, **kw)
    assert got == [cut(free[b], stops[b], eos) for b in range(8)]
    assert ST.finish_reason(got[1], ST.check_stop(stops[1], NEW, TAB), TAB, eos, NEW) == ("eos", None)


# ---------------------------------------------------------------------------------------------------------------- 3. launch forms
def test_ids_do_not_depend_on_batch_slot_graph_or_bank():
    emb = embeds(8, CFG["hidden_size"])
    e, _ = make_engine(CFG, 5, max_batch=8)
    try:
        e.set_stop_vocab(TAB)
        free = gen(e, emb)
        stops = derived(free)
        a = gen(e, emb, stop=stops)
        assert a == [cut(free[b], stops[b]) for b in range(8)] and gen(e, emb, stop=stops) == a
        for b in (1, 2, 3, 4, 6):                                            # alone in slot 0 == in the batch at slot b
            assert gen(e, [emb[b]], stop=stops[b])[0] == a[b]
        perm = [3, 0, 7, 1, 6, 2, 5, 4]                                      # another slot, other neighbours
        p = gen(e, [emb[i] for i in perm], stop=[stops[i] for i in perm])
        assert [p[perm.index(i)] for i in range(8)] == a
    finally:
        e.close()
    e, _ = make_engine(CFG, 5, max_batch=8, use_graph=False)                 # eager launches
    try:
        e.set_stop_vocab(TAB)
        assert gen(e, emb, stop=stops) == a
    finally:
        e.close()
    from aurora_amd.engine import AuroraCapEngine
    from tests.util import rand_llm_weights
    e = AuroraCapEngine({"vit": None, "llm": CFG}, {"llm": rand_llm_weights(CFG, 5)}, max_frames=1, max_batch=8, max_ctx=512,
                        max_new_tokens=NEW, num_banks=2)
    try:
        e.set_stop_vocab(TAB)
        e.select_bank(1)
        assert gen(e, emb, stop=stops) == a
        e.select_bank(0)
        assert gen(e, emb, stop=stops) == a
    finally:
        e.close()


def stream_stop(x, k):
    """the k-th kind of record for a clip whose free run is x"""
    return [None, dict(token_ids=[x[2]]), dict(strings=[tb(x[3]) + tb(x[4])[:1]]), dict(max_new_tokens=2 + k % 3)][k % 4]


def test_caption_stream_slot_reuse_commits_and_front_end_graphs_equal_each_clip_alone():
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_caption_batch import VCFG, weights
    N = 10
    gen_ = torch.Generator().manual_seed(21)
    clips = [(torch.randn(2 + i % 2, 3, 56, 56, generator=gen_).half().cuda(), [1, 20 + i] + [-200, 30 + i] * (2 + i % 2) + [40 + i] * (1 + i % 3))
             for i in range(7)]
    e = AuroraCapEngine({"vit": VCFG, "llm": CFG}, weights(), max_frames=4, max_batch=3, max_ctx=512, max_new_tokens=N, spare_slots=2)
    try:
        e.set_stop_vocab(TAB)
        free = [e.caption_ids(px, ids, 0.5, N, eos_id=None) for px, ids in clips]
        # clips without stops first: the front-end graphs of their buckets are captured under the option's old value
        got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=None, check_every=4, overlap=True, front_graph=True))
        assert [got[i] for i in range(7)] == free and not e._stop_mode
        stops = [stream_stop(free[i], i) for i in range(7)]
        want = [cut(free[i], stops[i], n_new=N) for i in range(7)]
        assert sum(len(w) < N for w in want) >= 5
        assert [e.caption_ids(px, ids, 0.5, N, eos_id=None, stop=stops[i]) for i, (px, ids) in enumerate(clips)] == want
        assert e.caption_batch(clips[:3], 0.5, N, eos_id=None, stop=stops[:3]) == want[:3]
        for kw in (dict(overlap=True, front_graph=True), dict(overlap=True, front_graph=False), dict(overlap=False)):
            for check_every in (4, 2):
                got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=None, check_every=check_every, stop=lambda i: stops[i], **kw))
                assert [got[i] for i in range(7)] == want, (kw, check_every)
        one = dict(max_new_tokens=3)                                         # one dict for every clip of the stream
        got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=None, check_every=2, overlap=True, stop=one))
        assert [got[i] for i in range(7)] == [x[:3] for x in free]
        got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=None, check_every=4, overlap=True))          # no stops again, same ctx
        assert [got[i] for i in range(7)] == free
        # a record the host rejects is that clip's own error; the others go on
        errs = []
        bad = lambda i: dict(strings=["x" * 65]) if i == 2 else stops[i]      # noqa: E731
        for kw in (dict(overlap=True), dict(overlap=False)):
            got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=None, check_every=4, stop=bad, on_error=lambda i, ex: errs.append(i), **kw))
            assert sorted(got) == [0, 1, 3, 4, 5, 6] and all(got[i] == want[i] for i in got)
        assert errs == [2, 2]
    finally:
        e.close()


def test_sibling_front_ends_get_their_records():
    from tests.test_gpu_shared_prefix import ADJACENT, N, RATIO, engine, requests
    cs, keys = requests(ADJACENT)
    e = engine(3, 3, 1)
    try:
        e.set_stop_vocab(TAB)
        free = dict(e.caption_stream(cs, RATIO, N, eos_id=None, check_every=4, overlap=False, share_key=lambda i: keys[i]))
        free = [free[i] for i in range(len(cs))]
        stops = [stream_stop(free[i], i + 1) for i in range(len(cs))]
        want = [cut(free[i], stops[i], n_new=N) for i in range(len(cs))]
        assert sum(len(w) < N for w in want) >= 5
        for overlap in (False, True):
            got = dict(e.caption_stream(cs, RATIO, N, eos_id=None, check_every=4, overlap=overlap, share_key=lambda i: keys[i],
                                        stop=lambda i: stops[i]))
            assert [got[i] for i in range(len(cs))] == want, overlap
    finally:
        e.close()
    e = engine(9)
    try:
        e.set_stop_vocab(TAB)
        assert e.caption_batch(cs, RATIO, N, eos_id=None, share=keys, stop=stops) == want
        px = cs[0][0]
        assert e.caption_prompts(px, [ids for _, ids in cs[:3]], RATIO, N, eos_id=None, stop=stops[:3]) == want[:3]
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------- 4. unasked means unchanged
def test_unasked_means_unchanged():
    emb = embeds(4, CFG["hidden_size"], seed=2)
    e, _ = make_engine(CFG, 5, max_batch=4)
    try:
        plain = gen(e, emb)
        neutral = dict(token_ids=[], strings=[], max_new_tokens=0)
        assert gen(e, emb, stop=None) == plain and gen(e, emb, stop=neutral) == plain and gen(e, emb, stop=[None, neutral] * 2) == plain
        assert gen(e, emb, stop=dict(max_new_tokens=NEW)) == plain and not e._stop_mode             # the batch's own limit asks nothing
        with pytest.raises(ValueError):
            gen(e, emb, stop=dict(strings=["ab"]))                           # no byte table yet
        with pytest.raises(Exception):
            e.slot_stop(0, ST.records([None]))                               # the records do not exist before the option is on
        assert not e._stop_mode
        short = gen(e, emb, stop=[dict(max_new_tokens=2), None, None, dict(token_ids=[plain[3][1]])])
        assert e._stop_mode and [len(x) for x in short] == [2, NEW, NEW, len(cut(plain[3], dict(token_ids=[plain[3][1]])))]
        assert short[1:3] == plain[1:3]                                      # neutral neighbours of stopping slots
        assert gen(e, emb, stop=neutral) == plain and gen(e, emb) == plain   # the option on: neutral records
        e.set_stop_vocab(TAB)
        assert gen(e, emb) == plain and gen(e, emb, stop=dict(strings=["ZZ"])) == plain
        e.set_stop_vocab(None)
        assert gen(e, emb) == plain
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 5. neighbours
def test_logprobs_record_every_token_and_logit_rules_act_beside_a_stop(eng):
    emb = embeds(4, CFG["hidden_size"])
    free = gen(eng, emb, logprobs=2)
    ids = [r["ids"] for r in free]
    stops = [dict(token_ids=[ids[0][3]]), dict(strings=[tb(ids[1][2]) + tb(ids[1][3])[:2]]), dict(max_new_tokens=4), None]
    got = gen(eng, emb, logprobs=2, stop=stops)
    for b in range(4):
        want = cut(ids[b], stops[b])
        n = len(want)
        assert got[b]["ids"] == want and len(got[b]["token_logprobs"]) == n and got[b]["top_ids"].shape == (n, 2)      # the stop token included
        assert got[b]["token_logprobs"].tobytes() == free[b]["token_logprobs"][:n].tobytes()
        assert np.array_equal(got[b]["top_ids"], free[b]["top_ids"][:n])
    # logit rules change the ids; the stop then cuts THAT run where the definition says
    rules = dict(no_repeat_ngram_size=1)
    ruled = gen(eng, emb, logit_rules=rules)
    assert ruled != ids and all(len(set(x)) == NEW for x in ruled)
    stops = [dict(token_ids=[ruled[0][5]]), dict(strings=[tb(ruled[1][6])[-1:] + tb(ruled[1][7])]), dict(max_new_tokens=3), None]
    both = gen(eng, emb, logit_rules=rules, stop=stops)
    assert both == [cut(ruled[b], stops[b]) for b in range(4)] and [len(x) for x in both[:1] + both[2:]] == [6, 3, NEW] and len(both[1]) <= 8
    # min_new_tokens holds back the batch's EOS only: a stop id fires from the first token
    first = ids[0][0]
    assert gen(eng, emb[:1], eos=first, logit_rules=dict(min_new_tokens=5))[0][0] != first
    assert gen(eng, emb[:1], logit_rules=dict(min_new_tokens=5), stop=dict(token_ids=[first]))[0] == [first]


# ---------------------------------------------------------------------------------------------------------------------- 6. callers
def test_llm_generate_stop_strings_on_the_checkpoint_fixture(tmp_path):
    from transformers import AutoTokenizer
    from tests.test_gpu_sampling import _ckpt_model
    g = golden("g13_checkpoint_e2e.npz")
    m, src = _ckpt_model(tmp_path)
    try:
        tok = AutoTokenizer.from_pretrained(src)
        table = ST.token_bytes(tok, 320)
        m.visual_encoder.reset_tome_r(float(g["ratio"]))
        px = torch.from_numpy(g["pixel_values"]).cuda()
        data = {"pixel_values": px.unsqueeze(0), "input_ids": torch.from_numpy(g["input_ids"])}

        def run(**kw):
            return m.llm.generate(**m(data, mode="inference"), num_beams=1, max_new_tokens=12, **kw)[0].tolist()
        plain = run(eos_token_id=None)
        text = b"".join(ST.bytes_of(table, t) for t in plain[:5])
        word = text[-3:].decode()                                            # ends with token 4
        want = plain[:ST.first_stop(plain, dict(strings=[word.encode()]), table, None, 12)]
        assert 1 <= len(want) <= 5
        assert run(eos_token_id=None, stop_strings=[word], tokenizer=tok) == want
        assert run(eos_token_id=None, stop_strings=word, tokenizer=tok) == want
        assert tok.decode(want).endswith(word) or word in tok.decode(want)   # the string stays in the output
        with pytest.raises(ValueError):
            run(eos_token_id=None, stop_strings=[word])                      # transformers needs the tokenizer too
        assert run(eos_token_id=[plain[6], plain[2], plain[4]]) == plain[:ST.first_stop(plain, dict(token_ids=[plain[2], plain[4]]), table, plain[6], 12)]
        assert run(eos_token_id=None, stop_token_ids=[plain[3]]) == plain[:ST.first_stop(plain, dict(token_ids=[plain[3]]), table, None, 12)]
        assert run(eos_token_id=None) == plain
        ids = g["input_ids"][0].tolist()
        assert m.caption_batch([(px, ids)], max_new_tokens=12, eos_token_id=None, stop=dict(strings=[word])) == [want]
    finally:
        m.engine.close()


def test_plugin_honor_until_on_the_real_engine(tmp_path):
    from types import SimpleNamespace
    from transformers import AutoTokenizer
    from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
    from tests.test_gpu_sampling import _ckpt_model
    m, src = _ckpt_model(tmp_path, max_batch=2)
    try:
        tok = AutoTokenizer.from_pretrained(src, padding_side="right")
        table = ST.token_bytes(tok, 320)

        def pre(frames):                                                  # frames [f, H, W, 3] uint8 -> [f, 3, 56, 56] fp16
            x = frames.permute(0, 3, 1, 2).float() / 255.0
            return torch.nn.functional.interpolate(x, size=(56, 56), mode="bilinear").half()
        frames = np.random.default_rng(3).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
        docs = {i: frames for i in range(3)}
        captured = []
        deliver = m.caption_stream

        def spy(*a, **kw):                                                # the ids behind the decoded text
            for k, ids in deliver(*a, **kw):
                captured.append((kw.get("stop"), list(ids)))
                yield k, ids
        m.caption_stream = spy
        m.llm.eos_token_id = None

        def plugin(**kw):
            p = P.AuroraCapMI355X(pretrained="unused", device="cuda", batch_size=2, _model=m, _tokenizer=tok, _preprocessor=pre, **kw)
            p.task_dict = {"t": {"s": docs}}
            return p

        def reqs(gen_kwargs):
            return [SimpleNamespace(args=("describe it", dict(gen_kwargs), lambda d: [d], i, "t", "s")) for i in range(3)]
        full_text = plugin().generate_until(reqs({"max_new_tokens": 8}))[0]
        caption = captured[0][1]
        assert len(captured) == 3 and all(s is None and ids == caption for s, ids in captured) and len(caption) == 8
        text = b"".join(ST.bytes_of(table, t) for t in caption[:4])
        word = text[-2:].decode()
        n = ST.first_stop(caption, dict(strings=[word.encode()]), table, None, 8)
        assert 1 <= n <= 4
        until = {"max_new_tokens": 8, "until": [word, "", "</s>"]}
        captured.clear()
        assert plugin().generate_until(reqs(until)) == [full_text] * 3       # honor_until off: dropped exactly as before
        assert all(s is None and ids == caption for s, ids in captured) and not m.engine._stop_mode
        captured.clear()
        texts = plugin(honor_until=True).generate_until(reqs(until))
        assert all(ids == caption[:n] for _, ids in captured) and len(captured) == 3                # stopped early on the device ...
        assert all(s == dict(token_ids=(), strings=(word.encode(),), max_new_tokens=0) for s, _ in captured)
        assert texts == [tok.decode(caption[:n], skip_special_tokens=True).split(word)[0]] * 3      # ... and the text is cut before the string
        assert all(word not in t for t in texts) and texts[0] != full_text
        captured.clear()
        plugin().generate_until(reqs({"max_new_tokens": 8, "stop_token_ids": [caption[2]]}))
        assert all(ids == caption[:ST.first_stop(caption, dict(token_ids=[caption[2]]), table, None, 8)] for _, ids in captured) and len(captured) == 3
        with pytest.raises(ValueError):
            plugin(honor_until=True).generate_until(reqs({"until": ["x" * 65]}))
    finally:
        m.engine.close()


def test_cli_stop():
    from transformers import AutoTokenizer
    fixture = os.path.join(ROOT, "tests", "golden", "ckpt_tiny")
    g = golden("g14_cli_e2e.npz")
    tok = AutoTokenizer.from_pretrained(fixture)
    table = ST.token_bytes(tok, 320)
    ids = g["ids"].tolist()
    word = b"".join(ST.bytes_of(table, t) for t in ids[:4])[-3:]
    n = ST.first_stop(ids, dict(strings=[word]), table, None, int(g["new"]))
    assert 1 <= n <= 4
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--model_path", fixture, "--visual_input", os.path.join(fixture, "clip.png"),
           "--prompt", str(g["prompt"]), "--token_kept_ratio", str(float(g["ratio"])), "--max_new_tokens", str(int(g["new"])),
           "--stop", word.decode(), "--stop", "never there"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = tok.batch_decode([ids[:n]], skip_special_tokens=True)[0]          # the decoded ids, stop string included
    assert r.stdout.rstrip("\n").endswith(want.rstrip("\n")) and str(g["text"]) not in r.stdout and word.decode() in want, (r.stdout[-500:], want)

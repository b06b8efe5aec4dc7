"""GPU: seeded sampling (sample_advance_kernel) against the package's own definition (aurora_amd/sampling.py, pinned to transformers'
warpers by tests/test_sampling_host.py): the pick alone on stored-seed rows, its draw statistics, and - through the engine - every
invariance the greedy path has, bit for bit on the ids: batch, slot, bank, hipGraph, slot reuse, prompt bucket, half grid.

The pick's criterion (`assert_pick`), for a row with parameters (T, k, p) and the draw u of (seed, stream, n): with eps = 4 x the
largest deviation of transformers' float32 pipeline from its float64 one on the 2560 rows (tests/golden/g18_sampling.npz), the kernel's
kept-set size must lie between the reference's sizes at p - eps and p + eps (equal to it where those agree, and always for top-k
alone), and u must lie in the token's interval of the float64 cumulative distribution over the kept set of that size, widened by eps."""
import os

import numpy as np
import pytest
import torch

from aurora_amd import sampling as S
from tests.sampling_cases import SETTINGS, chi2_stat, golden_cases, make_row
from tests.test_gpu_llm import LLM_CFGS, make_engine, padded
from tests.util import golden, observe

pytestmark = pytest.mark.gpu

EPS = 4.0 * float(golden("g18_sampling.npz")["f32_cdf_dev"])        # 4 x 1.4e-6
SEED, STREAM = 1234567890123, 5


def recs(T, k, p, n, seed=SEED, stream=STREAM):
    r = np.zeros(n, S.RECORD)
    r["temperature"], r["top_k"], r["top_p"], r["seed"], r["stream"] = T, k, p, seed, stream
    return r


def assert_pick(row, T, k, p, seed, stream, n, tok, kept, tag, stats=None):
    V = len(row)
    if T == 0:
        assert tok == int(np.argmax(row)), (tag, tok)
        return
    if p >= 1.0:
        m_lo = m_hi = int(S.kept_mask(row, T, k, 1.0).sum())                   # top-k alone: no arithmetic is involved
    else:
        m_lo = int(S.kept_mask(row, T, k, max(p - EPS, 1e-300)).sum())
        m_hi = int(S.kept_mask(row, T, k, min(p + EPS, 1.0)).sum())
    print(f"{tag}: kept {kept} reference [{m_lo}, {m_hi}] token {tok}")
    assert m_lo <= kept <= m_hi, (tag, kept, m_lo, m_hi)
    if stats is not None:
        stats["exact"] += m_lo == m_hi
        stats["rows"] += 1
    keep = S.top_set(row, int(kept))
    assert keep is not None, (tag, "the kept set splits equal values", kept)
    idx, lo, hi = S.cdf_intervals(row, T, keep)
    j = np.nonzero(idx == tok)[0]
    assert len(j) == 1, (tag, "token outside the kept set", tok)
    u = S.uniform(seed, stream, n)
    miss = max(lo[j[0]] - u, u - hi[j[0]], 0.0)
    print(f"{tag}: u {u!r} interval [{lo[j[0]]!r}, {hi[j[0]]!r}] miss {miss!r}")
    observe("sampling/draw_outside_f64_cdf_interval", miss, EPS)


@pytest.fixture(scope="module")
def eng():
    e, _ = make_engine(LLM_CFGS["hd32"], 5, max_batch=8, max_new=24)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------------------- 5. the pick alone
@pytest.mark.parametrize("stage", [1, 0])
def test_pick_on_the_stored_seed_rows(eng, stage):
    """all 2560 rows with the row staged in LDS; every 4th of them with the row re-read from global memory (same code otherwise)"""
    eng.set_option("sample_stage", stage)
    try:
        cases = golden_cases()[::1 if stage else 4]
        stats = {"exact": 0, "rows": 0}
        for c0 in range(0, len(cases), 128):
            chunk = cases[c0:c0 + 128]
            rows = np.stack([make_row(seed, sigma) for _, seed, sigma, _ in chunk])
            r = np.zeros(len(chunk), S.RECORD)
            for j, (i, _, _, (T, k, p)) in enumerate(chunk):
                r[j] = (T, p, k, STREAM + i % 3, SEED + i)
            tok, kept = eng.sample_rows(torch.from_numpy(rows).cuda(), r, [i % 50 for i, _, _, _ in chunk])
            for j, (i, seed, sigma, (T, k, p)) in enumerate(chunk):
                assert_pick(rows[j], T, k, p, SEED + i, STREAM + i % 3, i % 50, int(tok[j]), int(kept[j]), f"row{i}/stage{stage}", stats)
        assert stats["exact"] * 2 >= stats["rows"], stats               # the exact case is exercised on at least half of the rows
    finally:
        eng.set_option("sample_stage", 1)


@pytest.mark.parametrize("vocab", [320, 323, 32000, 40000])
def test_pick_edge_cases(eng, vocab):
    """unaligned vocabularies, k >= vocab, k = 1, p so small that one token stays, a repeated maximum, T = 0.05, T = 0 beside
    sampled rows, +-large logits, a vocabulary too large for the LDS stage (40000: the row is re-read from global memory)"""
    settings = SETTINGS + [(0.05, 0, 0.9), (0.05, 50, 1.0), (1.0, 1, 1.0), (1.0, vocab, 0.8), (1.0, vocab + 7, 1.0), (1.0, 0, 1e-9),
                           (0.0, 5, 0.5), (1.0, 0, 1.0), (3.0, 0, 0.999)]
    base = np.stack([make_row(900 + i, (2.0, 4.0)[i % 2], vocab) for i in range(6)])
    base[3, [17, 200, vocab - 1]] = base[3].max()                        # a repeated maximum
    base[4] *= 40.0                                                      # +-600: exp underflows for nearly the whole row
    base[5, ::3] = -np.inf                                               # masked-out tokens
    lg = torch.from_numpy(base).cuda()
    for T, k, p in settings:
        tok, kept = eng.sample_rows(lg, recs(T, k, p, 6), list(range(6)))
        for j in range(6):
            assert_pick(base[j], T, k, p, SEED, STREAM, j, int(tok[j]), int(kept[j]), f"v{vocab}/{(T, k, p)}/row{j}")
    # clamps of values the host cannot see: negative temperature = greedy, top_p > 1 / top_k < 0 = off, top_p <= 0 = the maximum alone
    tok, kept = eng.sample_rows(lg[:3], recs(-1.0, 5, 0.5, 3), [0, 1, 2])
    assert tok.tolist() == base[:3].argmax(1).tolist()
    tok, kept = eng.sample_rows(lg[:3], recs(1.0, -4, 1.5, 3), [0, 1, 2])
    assert kept.tolist() == [vocab] * 3
    tok, kept = eng.sample_rows(lg[:3], recs(1.0, 0, -0.5, 3), [0, 1, 2])
    assert kept.tolist() == [1, 1, 1] and tok.tolist() == base[:3].argmax(1).tolist()


def test_pick_is_a_function_of_row_and_counter_only(eng):
    """the same row in another block, with other rows around it, twice: the same token"""
    rows = np.stack([make_row(300 + i, 4.0) for i in range(8)])
    r = recs(1.0, 0, 0.95, 8)
    a = eng.sample_rows(torch.from_numpy(rows).cuda(), r, [3] * 8)
    b = eng.sample_rows(torch.from_numpy(rows[::-1].copy()).cuda(), r, [3] * 8)
    c = eng.sample_rows(torch.from_numpy(rows).cuda(), r, [3] * 8)
    assert a[0].tolist() == b[0][::-1].tolist() == c[0].tolist() and a[1].tolist() == b[1][::-1].tolist()
    d = eng.sample_rows(torch.from_numpy(rows).cuda(), r, [4] * 8)
    assert d[0].tolist() != a[0].tolist()                               # another token index, another draw


# -------------------------------------------------------------------------------------------------------------- 6. the draw's statistics
@pytest.mark.parametrize("setting", [(0.7, 50, 0.9), (1.0, 0, 0.9), (1.5, 0, 0.5)])
def test_gpu_frequencies_follow_the_reference_probabilities(eng, setting):
    from scipy.stats import chi2
    T, k, p = setting
    row = make_row(424242, 4.0)
    keep = S.kept_mask(row, T, k, p)
    idx, lo, hi = S.cdf_intervals(row, T, keep)
    lg = torch.from_numpy(row).cuda()[None].expand(1024, -1).contiguous()          # the entry takes one logits row per output row
    r = recs(T, k, p, 1024)
    counts = np.zeros(len(row), np.int64)
    for launch in range(64):
        tok, kept = eng.sample_rows(lg, r, list(range(launch * 1024, (launch + 1) * 1024)))
        assert (kept == int(keep.sum())).all()
        counts += np.bincount(tok, minlength=len(row))
    assert counts[~keep].sum() == 0
    stat, dof = chi2_stat(counts[idx], hi - lo, 65536)
    print(f"chi2 {setting}: {stat:.1f} with {dof} degrees of freedom, quantile {chi2.ppf(1 - 1e-6, dof):.1f}")
    assert dof >= 1 and stat < chi2.ppf(1 - 1e-6, dof), (stat, dof)


# ----------------------------------------------------------------------------------------------------------------------- 7. tokens
def embeds(n, d, seed=0):
    return [torch.randn(40 + 7 * i, d, generator=torch.Generator().manual_seed(seed + i)).half().float() for i in range(n)]


def gen(e, emb, n_new=20, eos=None, **kw):
    return e.generate([padded(x) for x in emb], [x.shape[0] for x in emb], n_new, eos_id=eos, **kw)


@pytest.mark.parametrize("name", ["hd32", "hd128"])
def test_top_k_1_is_greedy_bitwise_and_a_greedy_slot_keeps_its_ids_beside_sampling_slots(name):
    cfg = LLM_CFGS[name]
    emb = embeds(4, cfg["hidden_size"])
    e0, _ = make_engine(cfg, 6, max_batch=4)
    try:
        greedy = gen(e0, emb)                                            # an engine that never leaves mode 0
    finally:
        e0.close()
    e, _ = make_engine(cfg, 6, max_batch=4)
    try:
        assert gen(e, emb, sampling=dict(temperature=0.8, top_k=1, top_p=1.0, seed=3)) == greedy
        assert gen(e, emb) == greedy                                     # greedy calls in mode 1: the T == 0 branch
        # slot 2 greedy (temperature 0 record) between sampling slots
        e.begin_batch(4, 20, None)
        r = S.records(dict(temperature=1.0, top_k=0, top_p=1.0, seed=9), [0, 1, 2, 3])
        r[2] = np.zeros(1, S.RECORD)[0]
        e.slot_sampling(0, r)
        for b, x in enumerate(emb):
            e.prefill(b, padded(x), x.shape[0])
        e.decode(19)
        out = e.outputs()
        assert out[2] == greedy[2] and out[0] != greedy[0]
    finally:
        e.close()


# -------------------------------------------------------------------------------------------------------------------- 8. invariance
def flat_cfg():
    """hd32 with a vocabulary of 320 and random weights: logits of a few units, so that sampling at T = 1 spreads over many tokens
    (tests/test_sampling_host.py rolls the reference out on the oracle's logits of this model: seeds and streams differ within 8 tokens)"""
    return LLM_CFGS["hd32"]


SP = dict(temperature=1.0, top_k=0, top_p=0.95, seed=11)


@pytest.mark.parametrize("eos", [None, "hit"])
def test_ids_do_not_depend_on_batch_slot_graph_bank_or_repetition(eos):
    cfg = flat_cfg()
    emb = embeds(8, cfg["hidden_size"])
    e, _ = make_engine(cfg, 5, max_batch=8)
    try:
        free = gen(e, emb, sampling=SP)
        eos_id = None if eos is None else free[3][6]                    # a token the sampled run really emits: the EOS is hit
        a = gen(e, emb, eos=eos_id, sampling=SP)
        if eos_id is not None:
            assert len(a[3]) <= 7 and a[3][-1] == eos_id and any(len(x) < 20 for x in a)
        assert gen(e, emb, eos=eos_id, sampling=SP) == a                # the same call twice
        for b in (0, 5):                                                # alone in slot 0 == in the batch at slot b
            assert gen(e, [emb[b]], eos=eos_id, sampling=SP, streams=[b])[0] == a[b]
        perm = [3, 0, 7, 1, 6, 2, 5, 4]                                 # another slot, other neighbours
        p = gen(e, [emb[i] for i in perm], eos=eos_id, sampling=SP, streams=perm)
        assert [p[perm.index(i)] for i in range(8)] == a
        other_seed = gen(e, emb, eos=eos_id, sampling=dict(SP, seed=12))
        other_stream = gen(e, emb, eos=eos_id, sampling=SP, streams=range(100, 108))
        assert all(x[:8] != y[:8] for x, y in zip(free, gen(e, emb, sampling=dict(SP, seed=12))))
        assert other_seed != a and other_stream != a
        e.set_option("decode_half_grid", 1)
        try:
            assert gen(e, emb, eos=eos_id, sampling=SP) == a
        finally:
            e.set_option("decode_half_grid", 0)
    finally:
        e.close()
    e, _ = make_engine(cfg, 5, max_batch=8, use_graph=False)           # eager launches
    try:
        assert gen(e, emb, eos=eos_id, sampling=SP) == a
    finally:
        e.close()
    from aurora_amd.engine import AuroraCapEngine
    from tests.util import rand_llm_weights
    e = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 5)}, max_frames=1, max_batch=8, max_ctx=512,
                        max_new_tokens=24, num_banks=2)
    try:
        e.select_bank(1)
        assert gen(e, emb, eos=eos_id, sampling=SP) == a
        e.select_bank(0)
        assert gen(e, emb, eos=eos_id, sampling=SP) == a
    finally:
        e.close()


def test_half_grid_graph_of_a_128_slot_engine_gives_the_same_sampled_ids():
    """engines of more than 64 slots really launch the half-grid projections under decode_half_grid"""
    cfg = flat_cfg()
    emb = embeds(70, cfg["hidden_size"])
    e, _ = make_engine(cfg, 5, max_batch=128, max_ctx=640)
    try:
        a = gen(e, emb, n_new=12, sampling=SP)
        e.set_option("decode_half_grid", 1)
        try:
            assert gen(e, emb, n_new=12, sampling=SP) == a
        finally:
            e.set_option("decode_half_grid", 0)
        assert gen(e, [emb[66]], n_new=12, sampling=SP, streams=[66])[0] == a[66]
    finally:
        e.close()


@pytest.mark.parametrize("eos", [None, "hit"])
@pytest.mark.parametrize("bucket", [0, 32])
def test_caption_stream_slot_reuse_in_every_form_equals_each_clip_alone(bucket, eos):
    """eos "hit": an id the sampled alone runs emit within their first five tokens on some clips and not on others, so slots are freed
    early and re-filled (new stream, n = 0) while their neighbours are in the middle of a caption"""
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_caption_batch import VCFG, weights
    N = 10
    gen_ = torch.Generator().manual_seed(21)
    clips = [(torch.randn(2 + i % 2, 3, 56, 56, generator=gen_).half().cuda(), [1, 20 + i] + [-200, 30 + i] * (2 + i % 2) + [40 + i] * (1 + i % 3))
             for i in range(7)]
    e = AuroraCapEngine({"vit": VCFG, "llm": LLM_CFGS["hd32"]}, weights(), max_frames=4, max_batch=3, max_ctx=512, max_new_tokens=N,
                        spare_slots=2, prompt_bucket=bucket)
    try:
        free = [e.caption_ids(px, ids, 0.5, N, eos_id=None, sampling=SP, stream=i) for i, (px, ids) in enumerate(clips)]
        eos_id = None
        if eos is not None:
            # the token that cuts the most clips short within five tokens while leaving at least two at full length
            cands = sorted({t for x in free for t in x[:5]}, key=lambda t: (-sum(t in x[:5] for x in free), t))
            eos_id = next(t for t in cands if sum(t in x for x in free) <= 5)
        alone = [e.caption_ids(px, ids, 0.5, N, eos_id=eos_id, sampling=SP, stream=i) for i, (px, ids) in enumerate(clips)]
        if eos is not None:
            assert alone == [x[:x.index(eos_id) + 1] if eos_id in x else x for x in free]
            assert any(len(x) <= 5 for x in alone) and sum(len(x) == N for x in alone) >= 2, [len(x) for x in alone]
        greedy = [e.caption_ids(px, ids, 0.5, N, eos_id=eos_id) for px, ids in clips]
        assert alone != greedy
        assert e.caption_batch(clips[:3], 0.5, N, eos_id=eos_id, sampling=SP) == alone[:3]
        for kw in (dict(overlap=False), dict(overlap=True, front_graph=False), dict(overlap=True, front_graph=True)):
            for check_every in (4, 2):
                got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=eos_id, check_every=check_every, sampling=SP, **kw))
                assert [got[i] for i in range(7)] == alone, (kw, check_every)
        got = dict(e.caption_stream(iter(clips), 0.5, N, eos_id=eos_id, check_every=4, overlap=True))      # greedy again, same ctx
        assert [got[i] for i in range(7)] == greedy
    finally:
        e.close()
    if bucket:                                                          # prompt_bucket on == off
        e = AuroraCapEngine({"vit": VCFG, "llm": LLM_CFGS["hd32"]}, weights(), max_frames=4, max_batch=3, max_ctx=512, max_new_tokens=N)
        try:
            assert [e.caption_ids(px, ids, 0.5, N, eos_id=eos_id, sampling=SP, stream=i) for i, (px, ids) in enumerate(clips)] == alone
        finally:
            e.close()


# ------------------------------------------------------------------------------------------------------------- 9. audit of the wiring
def test_every_emitted_token_satisfies_the_criterion_on_the_gpus_own_logits():
    cfg = flat_cfg()
    emb = embeds(3, cfg["hidden_size"], seed=50)
    e, _ = make_engine(cfg, 5, max_batch=3, max_new=16)
    try:
        sp = dict(temperature=0.9, top_k=40, top_p=0.9, seed=77)
        streams = [4, 9, 2]
        e._sampling_on()
        e.begin_batch(3, 16, None)
        e.slot_sampling(0, S.records(S.check_sampling(sp), streams))
        for b, x in enumerate(emb):
            e.prefill(b, padded(x), x.shape[0])
        logits = [e.logits().cpu().numpy()]
        for _ in range(15):
            e.decode(1)
            logits.append(e.logits().cpu().numpy())
        out = e.outputs()
        # slot 1 is re-filled with another request: the counter restarts at 0 with the new stream
        e.slot_reset(1)
        e.slot_sampling(1, S.records(S.check_sampling(sp), [31]))
        e.prefill(1, padded(emb[2]), emb[2].shape[0])
        again = [e.logits().cpu().numpy()[1]]
        for _ in range(3):
            e.decode(1)
            again.append(e.logits().cpu().numpy()[1])
        out2 = e.outputs()
    finally:
        e.close()
    for b in range(3):
        assert len(out[b]) == 16
        for n in range(16):
            kept = int(S.kept_mask(logits[n][b], sp["temperature"], sp["top_k"], sp["top_p"]).sum())
            keep = S.top_set(logits[n][b], kept)
            idx, lo, hi = S.cdf_intervals(logits[n][b], sp["temperature"], keep)
            j = np.nonzero(idx == out[b][n])[0]
            assert len(j) == 1, (b, n)
            u = S.uniform(sp["seed"], streams[b], n)
            observe("sampling/engine_draw_outside_f64_cdf_interval", max(lo[j[0]] - u, u - hi[j[0]], 0.0), EPS)
    for n in range(4):
        kept = int(S.kept_mask(again[n], sp["temperature"], sp["top_k"], sp["top_p"]).sum())
        idx, lo, hi = S.cdf_intervals(again[n], sp["temperature"], S.top_set(again[n], kept))
        j = np.nonzero(idx == out2[1][n])[0]
        assert len(j) == 1, n
        u = S.uniform(sp["seed"], 31, n)
        observe("sampling/engine_draw_outside_f64_cdf_interval", max(lo[j[0]] - u, u - hi[j[0]], 0.0), EPS)


# ------------------------------------------------------------------------------------------------------- 10. the public ways in
def _ckpt_model(tmp_path, max_batch=1):
    from aurora_amd.model import AuroraModel
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_tiny")
    root = str(tmp_path / "ckpt")
    os.makedirs(root)
    for f in os.listdir(src):
        if not f.startswith("visual_encoder"):
            os.symlink(os.path.join(src, f), os.path.join(root, f))
    os.symlink(os.path.join(src, "visual_encoder_hf5"), os.path.join(root, "visual_encoder"))
    return AuroraModel.from_pretrained(root, max_frames=4, max_batch=max_batch, max_ctx=256, max_new_tokens=12), src


def test_llm_generate_do_sample_on_the_checkpoint_fixture(tmp_path):
    g = golden("g13_checkpoint_e2e.npz")
    m, _ = _ckpt_model(tmp_path)
    try:
        m.visual_encoder.reset_tome_r(float(g["ratio"]))
        data = {"pixel_values": torch.from_numpy(g["pixel_values"]).cuda().unsqueeze(0), "input_ids": torch.from_numpy(g["input_ids"])}

        def run(**kw):
            return m.llm.generate(**m(data, mode="inference"), num_beams=1, max_new_tokens=12, eos_token_id=None, **kw)[0].tolist()
        greedy = run(do_sample=False, temperature=0.7, top_p=0.9)
        a = run(do_sample=True, temperature=1.5, top_p=0.95, top_k=0, seed=4)
        assert a == run(do_sample=True, temperature=1.5, top_p=0.95, top_k=0, seed=4) and len(a) == 12
        assert a != greedy and a != run(do_sample=True, temperature=1.5, top_p=0.95, top_k=0, seed=5)
        assert run(do_sample=True, temperature=1.5, top_k=1) == greedy == run(do_sample=False)
        with pytest.raises(ValueError):
            run(do_sample=True, temperature=0.0)
        with pytest.raises(NotImplementedError):
            m.llm.generate(**m(data, mode="inference"), do_sample=True, temperature=1.0, num_beams=4)
    finally:
        m.engine.close()


def test_plugin_with_sampling_on_the_real_engine(tmp_path):
    from types import SimpleNamespace
    from transformers import AutoTokenizer
    from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
    m, src = _ckpt_model(tmp_path, max_batch=2)
    try:
        tok = AutoTokenizer.from_pretrained(src, padding_side="right")

        def pre(frames):                                                  # frames [f, H, W, 3] uint8 -> [f, 3, 56, 56] fp16
            x = frames.permute(0, 3, 1, 2).float() / 255.0
            return torch.nn.functional.interpolate(x, size=(56, 56), mode="bilinear").half()
        rng = np.random.default_rng(3)
        docs = {i: rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8) for i in range(5)}
        gens = [{"temperature": 1.5, "top_p": 0.95, "max_new_tokens": 8}, {"max_new_tokens": 8}] * 2 + [{"temperature": 1.5, "top_p": 0.95, "max_new_tokens": 8}]
        reqs = [SimpleNamespace(args=("describe " + "it " * i, gens[i], lambda d: [d], i, "t", "s")) for i in range(5)]

        def plugin(**kw):
            p = P.AuroraCapMI355X(pretrained="unused", device="cuda", batch_size=2, _model=m, _tokenizer=tok, _preprocessor=pre, **kw)
            p.task_dict = {"t": {"s": docs}}
            return p
        a = plugin(sampling=True, seed=7).generate_until(reqs)
        assert a == plugin(sampling=True, seed=7).generate_until(reqs) and len(a) == 5
        # a request's text depends on its index in `requests`, not on what else is asked: the sampled ones alone, reversed order of kinds
        only = plugin(sampling=True, seed=7).generate_until([reqs[0], reqs[1], reqs[2]])
        assert only == a[:3]
        b = plugin(sampling=True, seed=8).generate_until(reqs)
        assert [b[1], b[3]] == [a[1], a[3]] and [b[0], b[2], b[4]] != [a[0], a[2], a[4]]       # greedy requests stay greedy
        greedy_reqs = [SimpleNamespace(args=(r.args[0], {"max_new_tokens": 8}) + r.args[2:]) for r in reqs]
        g = plugin().generate_until(greedy_reqs)
        assert [g[1], g[3]] == [a[1], a[3]] and [g[0], g[2], g[4]] != [a[0], a[2], a[4]]
        with pytest.raises(NotImplementedError):
            plugin().generate_until(reqs)
    finally:
        m.engine.close()

"""GPU: the variable-length prefill (`aur_llm_prefill_*_var`: sequences a common stride apart, their lengths in device memory) gives
every sequence BITWISE what the single-sequence path `prefill(slot, embeds_i, len_i)` gives it in the same process - first token,
logits, every later decode step - whatever the padding rows held, and the two users of it (`caption_batch` groups by stride,
`caption_stream`'s captured front ends keyed by stride) give every clip the ids it gets alone.

No test here passes an out-of-range length in DEVICE memory: the kernels clamp such a value so that nothing faults, and that is not
something to provoke."""
import pytest
import torch

from tests.test_gpu_llm import LLM_CFGS, make_engine, padded

pytestmark = pytest.mark.gpu

NAN16, MAX16 = float("nan"), 65504.0                   # torch writes fp16 NaN as 0x7e00


def rand_embeds(cfg, lens, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(L, cfg["hidden_size"], generator=gen) * scale).half() for L in lens]


def strided(embs, stride, fill=0.0):
    """[nseq * stride, d] with sequence i at rows [i * stride, i * stride + len_i) and `fill` in every other row"""
    d = embs[0].shape[1]
    big = torch.full((len(embs) * stride, d), fill, dtype=torch.float16, device="cuda")
    for i, e in enumerate(embs):
        big[i * stride:i * stride + e.shape[0]] = e.cuda()
    return big


def run_alone(eng, embs, lens, steps):
    """the reference: every sequence through the existing single-sequence entry point into its own slot"""
    n = len(embs)
    eng.begin_batch(n, steps + 1, None)
    for b in range(n):
        eng.prefill(b, padded(embs[b].float()), lens[b])
    first = eng.logits()[:n].clone()
    eng.decode(steps)
    return first, eng.logits()[:n].clone(), eng.outputs()


def run_var(eng, embs, lens, stride, steps, fill=0.0, lens_dev=False):
    n = len(embs)
    eng.begin_batch(n, steps + 1, None)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens_dev else lens
    eng.prefill_batch(0, n, strided(embs, stride, fill), stride, seq_lens=sl)
    first = eng.logits()[:n].clone()
    eng.decode(steps)
    return first, eng.logits()[:n].clone(), eng.outputs()


def assert_same(got, want):
    assert got[2] == want[2]                                       # ids: first tokens and every decode step
    assert [x[0] for x in got[2]] == [x[0] for x in want[2]]
    assert torch.equal(got[0], want[0]), "logits of the last prompt positions differ"
    assert torch.equal(got[1], want[1]), "logits after the decode steps differ"


@pytest.mark.parametrize("name", ["hd32", "hd128"])
def test_four_lengths_at_stride_128_equal_each_sequence_alone(name):
    """lengths that cross round_up(len, 32) = 96 / 128 and a 64-token page"""
    cfg, lens = LLM_CFGS[name], [97, 128, 65, 111]
    embs = rand_embeds(cfg, lens, 50)
    eng, _ = make_engine(cfg, 21, max_batch=4, max_ctx=512, max_new=16)
    try:
        want = run_alone(eng, embs, lens, 12)
        assert_same(run_var(eng, embs, lens, 128, 12), want)
        assert_same(run_var(eng, embs, lens, 128, 12, lens_dev=True), want)      # lengths handed over as a device tensor
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["hd32", "hd128"])
@pytest.mark.parametrize("stride,lens", [(256, [129, 256, 200, 193]), (192, [190, 100, 190, 161])])
def test_pruned_last_layer_with_a_row0_per_sequence(name, stride, lens):
    """stride > 128: the last layer runs on each sequence's own last 128 rows (3 - 4 pages); a 100-row sequence in such a group uses
    row0 = 0.  The unpruned variable-length pass must agree too (`prefill_prune_last` is bit-neutral)."""
    cfg = LLM_CFGS[name]
    embs = rand_embeds(cfg, lens, 51)
    eng, _ = make_engine(cfg, 22, max_batch=4, max_ctx=512, max_new=16)
    try:
        want = run_alone(eng, embs, lens, 12)
        assert_same(run_var(eng, embs, lens, stride, 12), want)
        eng.set_option("prefill_prune_last", 0)
        assert_same(run_var(eng, embs, lens, stride, 12), want)
        eng.set_option("prefill_prune_last", 1)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["hd32", "hd128"])
def test_short_sequences_inside_a_group_that_really_prunes(name):
    """The toy configurations prune only from 288 / 320 rows on (the compact scratch must fit): stride 320, with sequences of 100 rows
    (row0 = 0), 190 (row0 = 64) and 289 / 300 (row0 = 192) in one pass.  Bitwise each sequence alone (which is unpruned for the short
    ones), bitwise the unpruned variable-length pass, and the pruning did happen: rows in front of a long sequence's block stop one
    layer early while its last prompt row is the full result."""
    cfg, stride, lens = LLM_CFGS[name], 320, [100, 300, 289, 190]
    embs = rand_embeds(cfg, lens, 57)
    eng, _ = make_engine(cfg, 26, max_batch=4, max_ctx=512, max_new=16)
    try:
        want = run_alone(eng, embs, lens, 12)
        bufs = {}
        for prune in (1, 0):
            eng.set_option("prefill_prune_last", prune)
            assert_same(run_var(eng, embs, lens, stride, 12, fill=NAN16), want)
            eng.begin_batch(4, 13, None)
            bufs[prune] = strided(embs, stride, NAN16)
            eng.prefill_batch(0, 4, bufs[prune], stride, seq_lens=lens)
            torch.cuda.synchronize()
        eng.set_option("prefill_prune_last", 1)
        a, b = bufs[1].view(4, stride, -1), bufs[0].view(4, stride, -1)
        for i, L in enumerate(lens):
            assert torch.equal(a[i, L - 1], b[i, L - 1]), i           # the row the first token is read from
            assert not a[i, L:].any() and not b[i, L:].any(), i        # padding rows: cleared, and zero after every layer
        assert not torch.equal(a[1, :192], b[1, :192]) and not torch.equal(a[3, :64], b[3, :64])
        assert torch.equal(a[0, :100], b[0, :100])                     # a block that starts at row 0 is the whole sequence
    finally:
        eng.close()


@pytest.mark.parametrize("stride,lens", [(128, [97, 128, 65, 111]), (256, [129, 256, 200, 193])])
def test_padding_rows_are_dont_care(stride, lens):
    """zeros, fp16 NaN and the largest finite fp16 in rows [len, stride): the same results, also 40 decode steps later - past the
    32-token V^T fragment that straddled the end of each prompt"""
    cfg = LLM_CFGS["hd32"]
    embs = rand_embeds(cfg, lens, 52)
    eng, _ = make_engine(cfg, 23, max_batch=4, max_ctx=512, max_new=48)
    try:
        want = run_alone(eng, embs, lens, 40)
        for fill in (0.0, NAN16, MAX16):
            assert_same(run_var(eng, embs, lens, stride, 40, fill=fill), want)
    finally:
        eng.close()


def test_stage_and_commit_beside_live_captions():
    from aurora_amd.engine import AuroraCapEngine
    from tests.util import rand_llm_weights
    cfg = LLM_CFGS["hd64"]
    eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 24)}, max_frames=1, max_batch=4, max_ctx=512,
                          max_new_tokens=20, spare_slots=2)
    try:
        old_lens, new_lens, N = [70, 150, 90, 40], [97, 111], 20
        old, new = rand_embeds(cfg, old_lens, 53), rand_embeds(cfg, new_lens, 54)
        alone = [eng.generate([padded(e.float())], [L], N, eos_id=None)[0] for e, L in zip(old + new, old_lens + new_lens)]
        eng.begin_batch(4, N, None)
        for b in range(4):
            eng.prefill(b, padded(old[b].float()), old_lens[b])
        eng.decode(6)
        buf = strided(new, 128, fill=NAN16)
        lens_dev = torch.tensor(new_lens, dtype=torch.int32, device="cuda")
        eng.prefill_stage(4, 2, buf, 128, seq_lens=lens_dev)        # into the spare sequences: no decode state is touched
        eng.decode(4)
        mid = eng.outputs()
        assert [x[:11] for x in alone[:4]] == mid
        eng.prefill_commit(2, 2, 4, buf, 128, seq_lens=lens_dev)    # slots 2, 3 take over the staged pages
        eng.decode(N - 1)
        out = eng.outputs()
        assert out[0] == alone[0] and out[1] == alone[1]            # the live captions never noticed
        assert out[2] == alone[4] and out[3] == alone[5]
    finally:
        eng.close()


def test_llama_7b_width_at_stride_2176():
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_configs import LLAMA_7B_WIDTH as cfg
    from tests.util import rand_llm_weights
    lens = [2113, 2142, 2176, 2150]
    embs = rand_embeds(cfg, lens, 55, scale=0.5)
    eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 3, wstd=0.02)}, max_frames=1, max_batch=4,
                          max_ctx=2560, max_new_tokens=16)
    try:
        want = run_alone(eng, embs, lens, 4)
        assert_same(run_var(eng, embs, lens, 2176, 4, fill=NAN16), want)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------- whole path
def cap_engine(max_batch, spare, prompt_bucket, max_new=12):
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_caption_batch import VCFG, weights
    return AuroraCapEngine({"vit": VCFG, "llm": LLM_CFGS["hd32"]}, weights(), max_frames=6, max_batch=max_batch, max_ctx=512,
                           max_new_tokens=max_new, spare_slots=spare, prompt_bucket=prompt_bucket)


def prompt_clips(frames, tails, seed):
    """clips of equal shape whose prompts end in `tails[i]` extra text tokens"""
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(frames, 3, 56, 56, generator=gen).half().cuda(), [1] + [-200, 30] * frames + [100 + (7 * i + j) % 150 for j in range(t)])
            for i, t in enumerate(tails)]


def strides_of(eng, cs, bucket):
    from aurora_amd.engine import prompt_stride, splice_rows, tokens_at_layer
    out = []
    for px, ids in cs:
        r = eng.tome_r(0.5, 56, 56)
        n_kept = tokens_at_layer(17, r, eng.v["num_hidden_layers"] - 1) - 1
        out.append(prompt_stride(splice_rows(ids, px.shape[0], n_kept)["seq_len"], bucket))
    return out


def count_calls(eng, name):
    calls, inner = [], getattr(eng, name)

    def wrapped(*a, **k):
        calls.append((a, k))
        return inner(*a, **k)
    setattr(eng, name, wrapped)
    return calls


def test_caption_batch_prefills_one_bucket_in_one_pass():
    tails = [1, 3, 4, 9, 15, 21]                                   # prompt lengths 1 .. 20 tokens apart
    cs = prompt_clips(3, tails, 60)
    got = {}
    for bucket in (64, 0):
        eng = cap_engine(6, 0, bucket)
        try:
            assert len(set(strides_of(eng, cs, 64))) == 1 and len(set(strides_of(eng, cs, 0))) == 6
            alone = [eng.caption_ids(px, ids, 0.5, 12, eos_id=None) for px, ids in cs]
            calls = count_calls(eng, "prefill_batch")
            got[bucket] = eng.caption_batch(cs, 0.5, 12, eos_id=None, prefill_group=8)
            assert got[bucket] == alone
            assert len(calls) == (1 if bucket else 6)
            if bucket:
                assert calls[0][1]["seq_lens"] is not None and calls[0][0][1] == 6
        finally:
            eng.close()
    assert got[64] == got[0]


def test_caption_stream_keeps_one_front_end_per_bucket_not_per_prompt():
    tails = [19, 1, 24, 20, 2, 18, 21, 3, 17, 4, 22, 16, 5, 15, 23, 6, 14, 7, 13, 8, 12, 9, 11, 10]      # long before short, both buckets
    cs = prompt_clips(4, tails, 61)
    eng = cap_engine(3, 2, 64)
    try:
        st = strides_of(eng, cs, 64)
        assert len(set(strides_of(eng, cs, 0))) == 24 and len(set(st)) == 2 and min(st.count(x) for x in set(st)) >= 4
        alone = {i: eng.caption_ids(px, ids, 0.5, 12, eos_id=None) for i, (px, ids) in enumerate(cs)}
        eager = dict(eng.caption_stream(cs, 0.5, 12, eos_id=None, check_every=4, front_graph=False))
        assert not eng._front_graphs
        captures = count_calls(eng, "graph_capture")
        got = dict(eng.caption_stream(cs, 0.5, 12, eos_id=None, check_every=4))
        assert got == eager == alone
        assert 2 <= len(eng._front_graphs) <= 2 * 2                 # buckets x spare sequences
        assert len(captures) == len(eng._front_graphs)
        again = dict(eng.caption_stream(cs, 0.5, 12, eos_id=None, check_every=5))
        assert again == alone and len(captures) == len(eng._front_graphs) <= 4      # nothing new was captured
    finally:
        eng.close()
    eng = cap_engine(3, 2, 0)                                     # exact lengths: a graph per prompt, up to the cap
    try:
        assert dict(eng.caption_stream(cs, 0.5, 12, eos_id=None, check_every=4)) == alone
        assert len(eng._front_graphs) == min(24, eng.front_graph_cap) == 16
    finally:
        eng.close()


def test_argument_errors_leave_the_ctx_usable():
    from aurora_amd._lib import AuroraHipError
    cfg, lens = LLM_CFGS["hd32"], [97, 128, 65, 111]
    embs = rand_embeds(cfg, lens, 56)
    eng, _ = make_engine(cfg, 25, max_batch=4, max_ctx=200, max_new=8)          # 4 pages of 64 = 256 positions per sequence
    try:
        want = run_alone(eng, embs, lens, 6)
        eng.begin_batch(4, 7, None)
        buf = strided(embs, 320)
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        L, st = eng.L, eng._stream()
        AUR_ERR_ARG = -1
        assert L.aur_llm_prefill_batch_var(eng.ctx, 0, 4, buf.data_ptr(), 100, ld.data_ptr(), st) == AUR_ERR_ARG         # stride % 32
        assert L.aur_llm_prefill_batch_var(eng.ctx, 0, 4, buf.data_ptr(), 320, ld.data_ptr(), st) == AUR_ERR_ARG         # beyond the pages
        assert L.aur_llm_prefill_batch_var(eng.ctx, 0, 4, buf.data_ptr(), 128, None, st) == AUR_ERR_ARG                  # null lengths
        assert b"seq_lens_dev" in L.aur_last_error(eng.ctx)
        assert L.aur_llm_prefill_batch_var(eng.ctx, 2, 4, buf.data_ptr(), 128, ld.data_ptr(), st) == AUR_ERR_ARG         # slots outside the batch
        assert L.aur_llm_prefill_stage_var(eng.ctx, 0, 4, buf.data_ptr(), 96 + 8, ld.data_ptr(), st) == AUR_ERR_ARG
        assert L.aur_llm_prefill_stage_var(eng.ctx, 3, 2, buf.data_ptr(), 128, ld.data_ptr(), st) == AUR_ERR_ARG         # no spare sequences here
        assert L.aur_llm_prefill_commit_var(eng.ctx, 0, 4, 0, buf.data_ptr(), 128, None, st) == AUR_ERR_ARG
        assert L.aur_llm_prefill_commit_var(eng.ctx, 0, 4, 0, buf.data_ptr(), 130, ld.data_ptr(), st) == AUR_ERR_ARG
        assert L.aur_project_splice_var(eng.ctx, None, 0, None, ld.data_ptr(), ld.data_ptr(), 4, 100, buf.data_ptr(), st) != 0
        with pytest.raises(ValueError):
            eng.prefill_batch(0, 4, buf, 128, seq_lens=[97, 129, 65, 111])      # len > stride
        with pytest.raises(ValueError):
            eng.prefill_batch(0, 4, buf, 256, seq_lens=[97, 194, 65, 111])      # len + max_new > max_ctx
        with pytest.raises(ValueError):
            eng.prefill_batch(0, 4, buf, 128, seq_lens=[97, 128, 65])           # one length per sequence
        with pytest.raises(AuroraHipError):
            eng.prefill_batch(0, 4, buf, 320, seq_lens=ld)
        torch.cuda.synchronize()
        assert_same(run_var(eng, embs, lens, 128, 6), want)                      # the ctx still works
    finally:
        eng.close()

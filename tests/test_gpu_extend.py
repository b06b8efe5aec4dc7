"""GPU: a prefill that starts at a position > 0 (`aur_llm_extend_*_var`) and the page copy that feeds it (`aur_kv_copy_prefix`).

The yardstick everywhere is the existing single-sequence path in the same process: a sequence whose first `pos0` positions were
written by a prefill (or copied from a sequence that holds them) and whose remaining rows went through `extend_*` has BITWISE the
first-token logits, the logits after the decode steps and the ids of `prefill(slot, full_embeds, pos0 + len)`.  No tolerance anywhere.

No test here passes an out-of-range value in DEVICE memory, and every rejected call is rejected on the host before anything is enqueued."""
import pytest
import torch

from tests.test_gpu_llm import LLM_CFGS, make_engine, padded
from tests.test_gpu_prefill_var import MAX16, NAN16, assert_same, rand_embeds, run_alone, strided

pytestmark = pytest.mark.gpu

# hd32 with a 4 x MLP: the pruned last layer needs 128 * (3 d + mlp) <= stride * mlp, which hd32 / hd128 reach at 320 / 288 rows only -
# with this one a stride of 256 prunes (the 7B shape, mlp = 2.7 d, prunes from 288 rows on)
WIDE = dict(LLM_CFGS["hd32"], intermediate_size=512)
CFGS = dict(LLM_CFGS, hd32w=WIDE)


def prunes(cfg, stride):
    """the rule of the layer stack (engine.hip prefill_layers): the compact scratch of the pruned last layer must fit"""
    return stride > 128 and 128 * (3 * cfg["hidden_size"] + cfg["intermediate_size"]) <= stride * cfg["intermediate_size"]


def stage_prefix(eng, embs, pos0):
    """positions [0, pos0) of every sequence, written by the existing call (the layer stack alone: no decode state is touched)"""
    for b, e in enumerate(embs):
        eng.prefill_stage(b, 1, padded(e[:pos0].float()), pos0)


def run_extend(eng, embs, pos0, stride, steps, fill=0.0, lens_dev=False):
    n, new = len(embs), [e[pos0:] for e in embs]
    lens = [e.shape[0] for e in new]
    eng.begin_batch(n, steps + 1, None)
    stage_prefix(eng, embs, pos0)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens_dev else lens
    eng.extend_batch(0, n, strided(new, stride, fill), pos0, stride, sl)
    first = eng.logits()[:n].clone()
    eng.decode(steps)
    return first, eng.logits()[:n].clone(), eng.outputs()


CASES = [(64, 64, [1, 33, 64, 17]),                   # one row, the 32-rounding, exactly one page
         (192, 256, [129, 256, 200, 193]),            # pos0 a multiple of 64 but not of 128
         (192, 320, [100, 300, 289, 190])]            # the stride from which hd32 / hd128 prune; row0 = 0, 192, 192, 64


@pytest.mark.parametrize("name", ["hd32", "hd128"])
@pytest.mark.parametrize("pos0,stride,new_lens", CASES)
def test_extend_equals_the_full_prefill(name, pos0, stride, new_lens):
    cfg = CFGS[name]
    full = [pos0 + x for x in new_lens]
    embs = rand_embeds(cfg, full, 70)
    eng, _ = make_engine(cfg, 31, max_batch=4, max_ctx=576, max_new=16)
    try:
        want = run_alone(eng, embs, full, 12)
        assert_same(run_extend(eng, embs, pos0, stride, 12), want)
        assert_same(run_extend(eng, embs, pos0, stride, 12, lens_dev=True), want)     # lengths handed over as a device tensor
        if prunes(cfg, stride):
            eng.set_option("prefill_prune_last", 0)
            assert_same(run_extend(eng, embs, pos0, stride, 12), want)
            eng.set_option("prefill_prune_last", 1)
    finally:
        eng.close()


@pytest.mark.parametrize("name,pos0,stride,new_lens", [("hd32w", 192, 256, [129, 256, 200, 193]), ("hd32", 192, 320, [100, 300, 289, 190]),
                                                       ("hd128", 192, 320, [100, 300, 289, 190])])
def test_extend_really_takes_the_pruned_last_layer(name, pos0, stride, new_lens):
    """The toy configurations hd32 / hd128 do not prune at a stride of 256 (see `prunes`), so that shape runs here on a wider MLP, and
    the two at the stride from which they do.  Pruned and unpruned extend are bitwise the full prefill; the pruning did happen: the
    rows in front of a long sequence's 128-row block stop one layer early while its last row is the full result, and the padding
    rows (filled with NaN by the caller) are zero after every layer."""
    cfg = CFGS[name]
    assert prunes(cfg, stride)
    full = [pos0 + x for x in new_lens]
    embs = rand_embeds(cfg, full, 71)
    eng, _ = make_engine(cfg, 32, max_batch=4, max_ctx=576, max_new=16)
    try:
        want = run_alone(eng, embs, full, 12)
        bufs = {}
        for prune in (1, 0):
            eng.set_option("prefill_prune_last", prune)
            assert_same(run_extend(eng, embs, pos0, stride, 12, fill=NAN16), want)
            eng.begin_batch(4, 13, None)
            stage_prefix(eng, embs, pos0)
            bufs[prune] = strided([e[pos0:] for e in embs], stride, NAN16)
            eng.extend_batch(0, 4, bufs[prune], pos0, stride, new_lens)
            torch.cuda.synchronize()
        eng.set_option("prefill_prune_last", 1)
        a, b = bufs[1].view(4, stride, -1), bufs[0].view(4, stride, -1)
        for i, L in enumerate(new_lens):
            assert torch.equal(a[i, L - 1], b[i, L - 1]), i
            assert not a[i, L:].any() and not b[i, L:].any(), i
        long = max(range(4), key=lambda i: new_lens[i])
        row0 = (new_lens[long] + 31) // 32 * 32 - 128
        assert row0 > 0 and not torch.equal(a[long, :row0], b[long, :row0])
        assert torch.equal(a[long, row0:new_lens[long]], b[long, row0:new_lens[long]])
    finally:
        eng.close()


@pytest.mark.parametrize("pos0,stride,new_lens", CASES[:2])
def test_padding_rows_are_dont_care(pos0, stride, new_lens):
    cfg = LLM_CFGS["hd32"]
    full = [pos0 + x for x in new_lens]
    embs = rand_embeds(cfg, full, 72)
    eng, _ = make_engine(cfg, 33, max_batch=4, max_ctx=576, max_new=48)
    try:
        want = run_alone(eng, embs, full, 40)             # past the 32-token V^T fragment that straddles the end of each prompt
        for fill in (NAN16, MAX16):
            assert_same(run_extend(eng, embs, pos0, stride, 40, fill=fill), want)
    finally:
        eng.close()


def with_tails(cfg, parent, pos0, tails, seed):
    """full sequences that share `parent`'s first pos0 rows and go on with their own rows"""
    return [torch.cat([parent[:pos0], t]) for t in rand_embeds(cfg, tails, seed)]


def test_copy_fan_out_from_a_live_parent():
    cfg, N = LLM_CFGS["hd64"], 20
    parent = rand_embeds(cfg, [150], 73)[0]
    tails = [1, 70, 37]
    kids = with_tails(cfg, parent, 128, tails, 74)
    eng, _ = make_engine(cfg, 34, max_batch=4, max_ctx=512, max_new=N)
    try:
        alone = [eng.generate([padded(e.float())], [e.shape[0]], N, eos_id=None)[0] for e in [parent] + kids]
        eng.begin_batch(4, N, None)
        for s in (1, 2, 3):
            eng.slot_retire(s)
        eng.prefill(0, padded(parent.float()), 150)
        eng.decode(5)                                     # the parent is live: positions 150 .. 154 are written beyond the copied pages
        eng.kv_copy_prefix(0, 1, 3, 128)
        for s in (1, 2, 3):
            eng.slot_reset(s)
        eng.extend_batch(1, 3, strided([k[128:] for k in kids], 96, NAN16), 128, 96, tails)
        eng.decode(N - 1)
        out = eng.outputs()
        assert out[1:] == alone[1:]
        assert out[0] == alone[0]                         # the parent never noticed
    finally:
        eng.close()


def test_stage_and_commit_beside_live_captions():
    from aurora_amd.engine import AuroraCapEngine
    from tests.util import rand_llm_weights
    cfg, N = LLM_CFGS["hd64"], 20
    eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 35)}, max_frames=1, max_batch=2, max_ctx=512,
                          max_new_tokens=N, spare_slots=3)
    try:
        old_lens = [100, 150]
        old = rand_embeds(cfg, old_lens, 75)
        tails = [45, 3]
        kids = with_tails(cfg, old[0], 64, tails, 76)
        alone = [eng.generate([padded(e.float())], [e.shape[0]], N, eos_id=None)[0] for e in old + kids]
        eng.begin_batch(2, N, None)
        for b in range(2):
            eng.prefill(b, padded(old[b].float()), old_lens[b])
        eng.decode(6)
        eng.kv_copy_prefix(0, 3, 2, 64)                   # from a decoding slot into the spare sequences 3, 4
        buf = strided([k[64:] for k in kids], 64, NAN16)
        lens_dev = torch.tensor(tails, dtype=torch.int32, device="cuda")
        eng.extend_stage(3, 2, buf, 64, 64, lens_dev)     # no decode state is touched
        eng.decode(4)
        assert eng.outputs() == [x[:11] for x in alone[:2]]
        eng.slot_retire(1)                                # slot 1's caption ends here; slot 0 keeps going
        eng.extend_commit(1, 1, 3, buf, 64, 64, lens_dev)
        eng.decode(N - 1)
        out = eng.outputs()
        assert out[0] == alone[0] and out[1] == alone[2]
        eng.extend_commit(0, 1, 4, buf[64:], 64, 64, lens_dev[1:])      # slot 0 has finished: the second staged child takes it
        eng.decode(N - 1)
        out = eng.outputs()
        assert out[0] == alone[3] and out[1] == alone[2]  # the neighbour's ids are unchanged
    finally:
        eng.close()


def test_sampled_extend_draws_what_the_plain_path_draws():
    from aurora_amd import sampling as S
    cfg, N = LLM_CFGS["hd32"], 16
    sp = dict(temperature=0.8, top_k=20, top_p=0.9, seed=3)
    lens = [64 + 33, 64 + 7]
    embs = rand_embeds(cfg, lens, 77)
    eng, _ = make_engine(cfg, 36, max_batch=2, max_ctx=512, max_new=N)
    try:
        want = eng.generate([padded(e.float()) for e in embs], lens, N, eos_id=None, sampling=sp, streams=[5, 9])
        greedy = eng.generate([padded(e.float()) for e in embs], lens, N, eos_id=None)
        assert want != greedy
        eng.begin_batch(2, N, None)
        eng.slot_sampling(0, S.records(S.check_sampling(sp), [5, 9]))
        stage_prefix(eng, embs, 64)
        eng.extend_batch(0, 2, strided([e[64:] for e in embs], 64), 64, 64, [33, 7])
        eng.decode(N - 1)
        assert eng.outputs() == want
    finally:
        eng.close()


def test_recorded_copy_and_stage_replayed_with_refilled_lengths():
    from aurora_amd.engine import AuroraCapEngine
    from tests.util import rand_llm_weights
    cfg, N = LLM_CFGS["hd32"], 12
    eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 37)}, max_frames=1, max_batch=2, max_ctx=512,
                          max_new_tokens=N, spare_slots=2)
    try:
        parent = rand_embeds(cfg, [140], 78)[0]
        rounds = [[40, 9], [1, 64]]
        kids = [with_tails(cfg, parent, 128, t, 79 + i) for i, t in enumerate(rounds)]
        alone = [[eng.generate([padded(e.float())], [e.shape[0]], N, eos_id=None)[0] for e in ks] for ks in kids]
        eng.begin_batch(2, N, None)
        eng.slot_retire(1)
        eng.prefill(0, padded(parent.float()), 140)
        buf = torch.zeros(2 * 64, cfg["hidden_size"], dtype=torch.float16, device="cuda")
        lens_dev = torch.ones(2, dtype=torch.int32, device="cuda")

        def front():
            eng.kv_copy_prefix(0, 2, 2, 128)
            eng.extend_stage(2, 2, buf, 128, 64, lens_dev)
        front()                                            # once eagerly: lazily set kernel attributes stay out of the capture
        gid, nodes = eng.graph_capture(front)
        assert nodes > 0
        for t, ks, want in zip(rounds, kids, alone):
            buf.copy_(strided([k[128:] for k in ks], 64, NAN16))
            lens_dev.copy_(torch.tensor(t, dtype=torch.int32))
            eng.graph_launch(gid)
            eng.extend_commit(0, 2, 2, buf, 128, 64, lens_dev)        # the exchange moves the pages; the next replay reads the table again
            eng.decode(N - 1)
            assert eng.outputs() == want
            eng.begin_batch(2, N, None)                    # the parent's positions again for the next round (slot 0 now owns other pages)
            eng.slot_retire(1)
            eng.prefill(0, padded(parent.float()), 140)
        eng.graph_destroy(gid)
    finally:
        eng.close()


def test_llama_7b_width_extends_30_rows_at_position_2112():
    """4096 wide, 1 MiB pages: slot 0 extends its own prefix, slot 1 a copy of it (33 pages x 2 layers through kv_copy_prefix_kernel)"""
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_configs import LLAMA_7B_WIDTH as cfg
    from tests.util import rand_llm_weights
    pos0, new = 2112, 30
    a = rand_embeds(cfg, [pos0 + new], 81, scale=0.5)[0]
    b = torch.cat([a[:pos0], rand_embeds(cfg, [new], 82, scale=0.5)[0]])
    eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 3, wstd=0.02)}, max_frames=1, max_batch=4,
                          max_ctx=2560, max_new_tokens=16)
    try:
        want = run_alone(eng, [a, b], [pos0 + new] * 2, 4)
        eng.begin_batch(2, 5, None)
        eng.prefill_stage(0, 1, padded(a[:pos0].float()), pos0)
        eng.kv_copy_prefix(0, 1, 1, pos0)
        eng.extend_batch(0, 2, strided([a[pos0:], b[pos0:]], 32, NAN16), pos0, 32, [new, new])
        first = eng.logits()[:2].clone()
        eng.decode(4)
        assert_same((first, eng.logits()[:2].clone(), eng.outputs()), want)
    finally:
        eng.close()


def test_argument_errors_leave_the_ctx_usable():
    from aurora_amd._lib import AuroraHipError
    cfg, pos0, new_lens = LLM_CFGS["hd32"], 64, [1, 33, 64, 17]
    full = [pos0 + x for x in new_lens]
    embs = rand_embeds(cfg, full, 83)
    eng, _ = make_engine(cfg, 38, max_batch=4, max_ctx=200, max_new=8)          # 4 pages of 64 = 256 positions per sequence, no spare ones
    try:
        want = run_alone(eng, embs, full, 6)
        eng.begin_batch(4, 7, None)
        buf = strided([e[pos0:] for e in embs], 256)
        ld = torch.tensor(new_lens, dtype=torch.int32, device="cuda")
        L, st, ERR = eng.L, eng._stream(), -1
        for bad in (0, 32, 96, -64):                                             # pos0: a positive multiple of 64
            assert L.aur_llm_extend_batch_var(eng.ctx, 0, 4, buf.data_ptr(), bad, 64, ld.data_ptr(), st) == ERR
            assert L.aur_llm_extend_stage_var(eng.ctx, 0, 4, buf.data_ptr(), bad, 64, ld.data_ptr(), st) == ERR
            assert L.aur_llm_extend_commit_var(eng.ctx, 0, 4, 0, buf.data_ptr(), bad, 64, ld.data_ptr(), st) == ERR
        assert b"pos0" in L.aur_last_error(eng.ctx)
        assert L.aur_llm_extend_batch_var(eng.ctx, 0, 4, buf.data_ptr(), 64, 256, ld.data_ptr(), st) == ERR     # pos0 + stride beyond the pages
        assert L.aur_llm_extend_batch_var(eng.ctx, 0, 4, buf.data_ptr(), 256, 32, ld.data_ptr(), st) == ERR
        assert L.aur_llm_extend_batch_var(eng.ctx, 0, 4, buf.data_ptr(), 64, 48, ld.data_ptr(), st) == ERR      # stride % 32
        assert L.aur_llm_extend_batch_var(eng.ctx, 0, 4, buf.data_ptr(), 64, 64, None, st) == ERR               # null lengths
        assert L.aur_llm_extend_batch_var(eng.ctx, 2, 4, buf.data_ptr(), 64, 64, ld.data_ptr(), st) == ERR      # slots outside the batch
        assert L.aur_llm_extend_stage_var(eng.ctx, 3, 2, buf.data_ptr(), 64, 64, ld.data_ptr(), st) == ERR      # no spare sequences here
        assert L.aur_llm_extend_commit_var(eng.ctx, 0, 4, 0, buf.data_ptr(), 64, 64, None, st) == ERR
        for tokens in (0, 1, 63, 65, 100, 320, -64):                             # a positive multiple of 64 within the pages
            assert L.aur_kv_copy_prefix(eng.ctx, 0, 1, 1, tokens, st) == ERR
        assert b"tokens" in L.aur_last_error(eng.ctx)
        assert L.aur_kv_copy_prefix(eng.ctx, 1, 0, 3, 64, st) == ERR             # source inside the destinations
        assert L.aur_kv_copy_prefix(eng.ctx, 0, 0, 1, 64, st) == ERR
        assert b"inside" in L.aur_last_error(eng.ctx)
        for src, dst0, ndst in ((4, 0, 1), (-1, 0, 1), (0, 4, 1), (0, 2, 3), (0, -1, 1), (0, 1, 0), (0, 1, -1)):      # ids out of range
            assert L.aur_kv_copy_prefix(eng.ctx, src, dst0, ndst, 64, st) == ERR
        with pytest.raises(ValueError):
            eng.extend_batch(0, 4, buf, 64, 64, [1, 65, 64, 17])                 # len > stride
        with pytest.raises(ValueError):
            eng.extend_batch(0, 4, buf, 192, 64, [1, 33, 64, 17])                # pos0 + len + max_new > max_ctx
        with pytest.raises(ValueError):
            eng.extend_batch(0, 4, buf, 64, 64, [1, 33, 64])                     # one length per sequence
        with pytest.raises(AuroraHipError):
            eng.extend_batch(0, 4, buf, 96, 64, ld)
        with pytest.raises(AuroraHipError):
            eng.kv_copy_prefix(0, 1, 3, 32)
        torch.cuda.synchronize()
        assert_same(run_extend(eng, embs, pos0, 64, 6), want)                    # the ctx still works
        eng.begin_batch(4, 7, None)                                              # and so does a valid copy
        stage_prefix(eng, embs[:1], pos0)
        eng.kv_copy_prefix(0, 1, 3, 64)
        eng.extend_batch(0, 4, strided([embs[0][pos0:]] * 4, 64), pos0, 64, [1] * 4)
        eng.decode(6)
        out = eng.outputs()
        assert out[0] == want[2][0] and out[1] == out[0] and out[2] == out[0] and out[3] == out[0]
    finally:
        eng.close()

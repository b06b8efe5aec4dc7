"""GPU parity: projector + splice, Llama prefill and greedy decode (paged KV, hipGraph), through the C ABI,
vs the CPU oracle.  Tolerances (SURVEY 8c iv): teacher-forced logits max-abs error relative to the logit
scale; greedy tokens must agree wherever the oracle's top-1 / top-2 margin exceeds twice that error."""
import numpy as np
import pytest
import torch

from oracle import aurora_oracle as O
from tests.util import observe, rand_llm_weights, rand_proj_weights, rand_vit_weights, rel_l2

pytestmark = pytest.mark.gpu

LLM_CFGS = {
    "hd32": dict(hidden_size=128, num_attention_heads=4, num_hidden_layers=2, intermediate_size=256, vocab_size=320,
                 rms_norm_eps=1e-5, rope_theta=1e4, rope_factor=4.0),
    "hd64": dict(hidden_size=256, num_attention_heads=4, num_hidden_layers=2, intermediate_size=384, vocab_size=500,
                 rms_norm_eps=1e-5, rope_theta=1e4, rope_factor=1.0),
    "hd128": dict(hidden_size=256, num_attention_heads=2, num_hidden_layers=3, intermediate_size=640, vocab_size=1000,
                  rms_norm_eps=1e-6, rope_theta=1e4, rope_factor=4.0),
}
# the greedy pick scans a row of logits with 1024 threads and 16-byte loads: a vocabulary that is not a multiple of 4 (scalar scan) and one
# that takes more than one pass of the block
LLM_CFGS_VOCAB = {
    "v323": dict(hidden_size=128, num_attention_heads=4, num_hidden_layers=1, intermediate_size=256, vocab_size=323,
                 rms_norm_eps=1e-5, rope_theta=1e4, rope_factor=1.0),
    "v9000": dict(hidden_size=128, num_attention_heads=4, num_hidden_layers=1, intermediate_size=256, vocab_size=9000,
                  rms_norm_eps=1e-5, rope_theta=1e4, rope_factor=1.0),
}
from tests.parity_bounds import FEAT_TOL, LOGIT_TOL  # noqa: E402  (max-abs relative to max |logit|; frozen from the observed errors)


def make_engine(cfg, seed, max_batch=2, use_graph=True, max_ctx=512, max_new=24):
    from aurora_amd.engine import AuroraCapEngine
    w = rand_llm_weights(cfg, seed)
    e = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": w}, max_frames=1, max_batch=max_batch, max_ctx=max_ctx,
                        max_new_tokens=max_new, use_graph=use_graph)
    return e, w


def padded(emb):
    L, d = emb.shape
    lp = (L + 31) // 32 * 32
    out = torch.zeros(lp, d, dtype=torch.float16, device="cuda")
    out[:L] = emb.half().cuda()
    return out


def assert_greedy_agrees_up_to_margin(got, ref_ids, ref_logits, tol=LOGIT_TOL):
    """The margin rule of this suite for free-running greedy decodes: tokens must equal the oracle's at every position up to
    the first one where the oracle's own top-1 / top-2 margin is inside twice the logit tolerance (past a legitimate flip the
    two sequences condition on different tokens and are no longer comparable).  Returns the number of positions checked."""
    scale = ref_logits.abs().max().item()
    checked = 0
    for i, (a, b) in enumerate(zip(got, ref_ids)):
        top2 = ref_logits[i].topk(2).values
        if (top2[0] - top2[1]).item() <= 2 * tol * scale:
            break
        assert a == b, (i, a, b, (top2[0] - top2[1]).item(), scale)
        checked += 1
    return checked


def teacher_forced_logits(emb, ids, w, cfg):
    """Oracle logits at every generated position given the GPU's own tokens."""
    full = torch.cat([emb, w["embed_tokens.weight"][torch.tensor(ids[:-1], dtype=torch.long)]], 0) if len(ids) > 1 else emb
    h, _ = O.llama_forward(full, w, cfg, None, 0)
    return torch.nn.functional.linear(h[emb.shape[0] - 1:], w["lm_head.weight"])


@pytest.mark.parametrize("name", list(LLM_CFGS) + list(LLM_CFGS_VOCAB))
@pytest.mark.parametrize("L", [40, 97])
def test_prefill_and_stepwise_decode_logits(name, L):
    cfg = LLM_CFGS.get(name) or LLM_CFGS_VOCAB[name]
    eng, w = make_engine(cfg, 5, max_batch=1, use_graph=False)
    try:
        gen = torch.Generator().manual_seed(L)
        emb = torch.randn(L, cfg["hidden_size"], generator=gen).half().float()
        nnew = 12
        eng.begin_batch(1, nnew, None)
        eng.prefill(0, padded(emb), L)
        logits = [eng.logits()[0].cpu()]
        for _ in range(nnew - 1):
            eng.decode(1)
            logits.append(eng.logits()[0].cpu())
        ids = eng.outputs()[0]
        assert len(ids) == nnew
        ref = teacher_forced_logits(emb, ids, w, cfg)
        scale = ref.abs().max().item()
        for i in range(nnew):
            err = (logits[i] - ref[i]).abs().max().item()
            observe(f"llm/stepwise_logits_max_err_over_scale[{name}]", err / scale, LOGIT_TOL)
            assert int(torch.argmax(logits[i])) == ids[i]                        # greedy = first argmax of the GPU logits
            top2 = ref[i].topk(2).values
            if (top2[0] - top2[1]).item() > 2 * LOGIT_TOL * scale:
                assert int(torch.argmax(ref[i])) == ids[i], i
    finally:
        eng.close()


def test_odd_vocabulary_logits_in_a_batch():
    """v323 (rows of logits end off the 16-byte grid) with three slots decoding together: every slot's logits - column 0 included, the
    address right behind the previous row's last column - against the oracle, and bitwise those of the slot decoded alone"""
    cfg = LLM_CFGS_VOCAB["v323"]
    lens, nnew = (40, 97, 33), 6
    gen = torch.Generator().manual_seed(11)
    embs = [torch.randn(L, cfg["hidden_size"], generator=gen).half().float() for L in lens]

    def stepwise(eng, which):
        eng.begin_batch(len(which), nnew, None)
        for slot, i in enumerate(which):
            eng.prefill(slot, padded(embs[i]), lens[i])
        logits = [eng.logits().cpu()]
        for _ in range(nnew - 1):
            eng.decode(1)
            logits.append(eng.logits().cpu())
        return torch.stack(logits, 1), eng.outputs()              # [slot, step, vocab]

    eng, w = make_engine(cfg, 5, max_batch=3, use_graph=False)
    try:
        together, ids = stepwise(eng, (0, 1, 2))
        for i in range(3):
            alone, ids1 = stepwise(eng, (i,))
            assert ids1[0] == ids[i]
            assert torch.equal(alone[0], together[i]), ("a slot's logits depend on its neighbours", i)
            ref = teacher_forced_logits(embs[i], ids[i], w, cfg)
            scale = ref.abs().max().item()
            observe("llm/odd_vocab_batched_logits_max_err_over_scale", (together[i] - ref).abs().max().item() / scale, LOGIT_TOL)
    finally:
        eng.close()


def test_greedy_matches_oracle_ids_and_graph_equals_eager():
    cfg = LLM_CFGS["hd128"]
    emb = torch.randn(50, cfg["hidden_size"], generator=torch.Generator().manual_seed(3)).half().float()
    outs = []
    for use_graph in (False, True):
        eng, w = make_engine(cfg, 6, max_batch=1, use_graph=use_graph)
        try:
            outs.append(eng.generate([padded(emb)], [50], 20, eos_id=None)[0])
        finally:
            eng.close()
    assert outs[0] == outs[1], "hipGraph replay must reproduce the eager decode bit for bit"
    ref_ids, ref_logits = O.llama_greedy(emb, w, cfg, 20, eos_id=None, return_logits=True)
    # agree up to the first position where the oracle's margin is inside the fp16 tolerance
    scale = ref_logits.abs().max().item()
    for i, (a, b) in enumerate(zip(outs[0], ref_ids)):
        top2 = ref_logits[i].topk(2).values
        if (top2[0] - top2[1]).item() <= 2 * LOGIT_TOL * scale:
            break
        assert a == b, i


def test_batched_ragged_decode_equals_single():
    """Slots with different prompt lengths decoded together give the same tokens as decoded alone."""
    cfg = LLM_CFGS["hd64"]
    gen = torch.Generator().manual_seed(8)
    embs = [torch.randn(L, cfg["hidden_size"], generator=gen).half().float() for L in (33, 70, 128)]
    eng, w = make_engine(cfg, 7, max_batch=3, use_graph=True)
    try:
        together = eng.generate([padded(e) for e in embs], [e.shape[0] for e in embs], 16, eos_id=None)
        alone = [eng.generate([padded(e)], [e.shape[0]], 16, eos_id=None)[0] for e in embs]
        assert together == alone
    finally:
        eng.close()


def test_eos_stops_and_lengths():
    cfg = LLM_CFGS["hd32"]
    emb = torch.randn(40, cfg["hidden_size"], generator=torch.Generator().manual_seed(4)).half().float()
    eng, w = make_engine(cfg, 9, max_batch=1, use_graph=True)
    try:
        free = eng.generate([padded(emb)], [40], 16, eos_id=None)[0]
        assert len(free) == 16
        eos = free[5]
        first = free.index(eos)
        stopped = eng.generate([padded(emb)], [40], 16, eos_id=eos, check_every=4)[0]
        assert stopped == free[: first + 1]          # generation ends with the EOS token itself (HF semantics)
    finally:
        eng.close()


def test_projector_splice_and_whole_path():
    from aurora_amd.engine import AuroraCapEngine
    vcfg = dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=4, intermediate_size=128, patch_size=14,
                image_size=56, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    lcfg = LLM_CFGS["hd32"]
    w = {"vit": rand_vit_weights(vcfg, 1), "projector": rand_proj_weights(64, lcfg["hidden_size"], 2),
         "llm": rand_llm_weights(lcfg, 3)}
    eng = AuroraCapEngine({"vit": vcfg, "llm": lcfg}, w, max_frames=3, max_batch=1, max_ctx=256, max_new_tokens=16)
    try:
        gen = torch.Generator().manual_seed(76)     # CPU search over the oracle alone: every one of the 12 steps has a clear margin at 1e-2
        px = torch.randn(3, 3, 56, 56, generator=gen).half().float()
        ids = [1, 17, -200, 18, -200, 19, -200, 20, 21, 22]
        # projector + splice alone (teacher-forced on the GPU's ViT features)
        r = eng.tome_r(0.5)
        vis = eng.vit_encode(px, r)
        emb, L = eng.project_splice(vis, ids)
        torch.cuda.synchronize()
        vis_ref = O.projector(vis.float().cpu().reshape(1, -1, 64), w["projector"]).reshape(3, vis.shape[1], -1)
        emb_ref = O.splice(torch.tensor(ids), w["llm"]["embed_tokens.weight"], vis_ref)
        assert L == emb_ref.shape[0] == 7 + 3 * vis.shape[1]
        observe("llm/whole_path_spliced_embeds_rel_l2", rel_l2(emb[:L].float().cpu(), emb_ref), FEAT_TOL)
        text_rows = [i for i, v in enumerate(emb_ref) if False]
        np.testing.assert_array_equal(emb[0].float().cpu().numpy(), w["llm"]["embed_tokens.weight"][1].numpy())   # text rows are exact copies
        # more markers than frames: the extra markers are dropped (utils.py:228-233)
        emb2, L2 = eng.project_splice(vis[:2], ids)
        assert L2 == 7 + 2 * vis.shape[1]
        # whole path, greedy ids vs oracle (fp16-storage emulation), up to the first inside-tolerance margin
        out = eng.caption_ids(px, ids, 0.5, 12, eos_id=None)
        assert len(out) == 12
        ref, ref_logits = O.caption_ids(px, ids, w, {"vit": vcfg, "llm": lcfg}, 0.5, 12, eos_id=None, q=O.fp16_storage, return_logits=True)
        # tolerance 1e-2 of the logit scale (tiny-model drift is well below the kernel-level 3e-2; at 3e-2 a random tiny model leaves
        # no position to compare) and the count is asserted: the check cannot pass vacuously
        checked = assert_greedy_agrees_up_to_margin(out, ref, ref_logits, 1e-2)
        assert checked >= 8, (checked, out, ref)
    finally:
        eng.close()


def test_reference_operator_seam_matches_engine_path():
    """reset_tome_r / model(data, mode='inference') / llm.generate(**output, ...) - the three calls of
    inference.py:87-96 - give the same ids as the engine's own whole-path call, and keep the error behaviour."""
    from aurora_amd.engine import AuroraCapEngine
    from aurora_amd.model import AuroraModel
    vcfg = dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=4, intermediate_size=128, patch_size=14,
                image_size=56, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    lcfg = LLM_CFGS["hd32"]
    w = {"vit": rand_vit_weights(vcfg, 1), "projector": rand_proj_weights(64, lcfg["hidden_size"], 2), "llm": rand_llm_weights(lcfg, 3)}
    eng = AuroraCapEngine({"vit": vcfg, "llm": lcfg}, w, max_frames=3, max_batch=1, max_ctx=256, max_new_tokens=16)
    try:
        m = AuroraModel(eng, eos_token_id=None)
        px = torch.randn(1, 3, 3, 56, 56, generator=torch.Generator().manual_seed(5)).half()
        ids = torch.tensor([[1, 17, -200, 18, -200, 19, -200, 20]])
        m.visual_encoder.reset_tome_r(0.5)
        out = m({"pixel_values": px, "input_ids": ids}, mode="inference")
        assert out["input_ids"] is None and out["attention_mask"] is None and out["position_ids"] is None and out["labels"] is None
        n_kept = out["inputs_embeds"].shape[1] - 5
        assert out["inputs_embeds"].shape[0] == 1 and n_kept % 3 == 0
        cont = m.llm.generate(**out, do_sample=False, temperature=0.0, top_p=1.0, num_beams=1, max_new_tokens=10)
        assert cont.dtype == torch.long and cont.shape == (1, 10)
        assert cont[0].tolist() == eng.caption_ids(px[0], ids[0].tolist(), 0.5, 10, eos_id=None)
        # single image [1, c, h, w] is a one-frame video (aurora.py:217-218)
        one = m({"pixel_values": px[:, 0], "input_ids": torch.tensor([[1, -200, 5]])}, mode="inference")
        assert one["inputs_embeds"].shape[1] == 2 + n_kept // 3
        with pytest.raises(NotImplementedError):
            m({"pixel_values": px, "input_ids": ids}, mode="bogus")
        with pytest.raises(NotImplementedError):
            m.llm.generate(**out, do_sample=False, num_beams=4, max_new_tokens=4)
    finally:
        eng.close()


def test_prefill_gemm256_equals_gemm128():
    """Llama prefill through the 256x256 kernel (RoPE + paged-KV epilogue) reproduces the 128x128 path's tokens/logits."""
    cfg = LLM_CFGS["hd128"]
    emb = torch.randn(300, cfg["hidden_size"], generator=torch.Generator().manual_seed(13)).half().float()
    eng, w = make_engine(cfg, 6, max_batch=1, use_graph=False)
    try:
        res = []
        for mode in (0, 2):
            eng.set_option("gemm_mode", mode)
            eng.begin_batch(1, 8, None)
            eng.prefill(0, padded(emb), 300)
            lg = eng.logits().clone()
            eng.decode(7)
            res.append((lg, eng.outputs()[0]))
        eng.set_option("gemm_mode", 1)
        assert torch.equal(res[0][0], res[1][0])
        assert res[0][1] == res[1][1]
    finally:
        eng.set_option("gemm_mode", 1)
        eng.close()


@pytest.mark.parametrize("name", ["hd32", "hd128"])
def test_single_split_decode_attention_finishes_in_the_kernel(name):
    """Engines whose batch alone fills the GPU run decode attention with ONE split per (sequence, head): the kernel then
    normalises and writes the x-fragment output itself and the combine launch disappears.  Forced here on a small engine
    (dec_attn_pps beyond the context); logits vs the oracle, hipGraph == eager, batch of ragged sequences == each alone."""
    cfg = LLM_CFGS[name]
    gen = torch.Generator().manual_seed(17)
    lens = [37, 150, 64]
    embs = [torch.randn(L, cfg["hidden_size"], generator=gen).half().float() for L in lens]
    outs = {}
    for use_graph in (False, True):
        eng, w = make_engine(cfg, 11, max_batch=3, use_graph=use_graph)
        try:
            eng.set_option("dec_attn_pps", 1 << 20)
            outs[use_graph] = eng.generate([padded(e) for e in embs], lens, 12, eos_id=None)
            if not use_graph:
                alone = [eng.generate([padded(e)], [L], 12, eos_id=None)[0] for e, L in zip(embs, lens)]
                assert outs[False] == alone
                eng.begin_batch(1, 6, None)
                eng.prefill(0, padded(embs[1]), lens[1])
                logits = [eng.logits()[0].cpu()]
                for _ in range(5):
                    eng.decode(1)
                    logits.append(eng.logits()[0].cpu())
                ids = eng.outputs()[0]
                ref = teacher_forced_logits(embs[1], ids, w, cfg)
                scale = ref.abs().max().item()
                for i in range(6):
                    observe("llm/batched_logits_max_err_over_scale", (logits[i] - ref[i]).abs().max().item() / scale, LOGIT_TOL)
        finally:
            eng.close()
    assert outs[False] == outs[True]


@pytest.mark.parametrize("name", ["hd32", "hd128"])
def test_decode_attention_against_the_oracle_split_counts_graph_and_batch(name):
    """The decode attention (v_dot2c page pipeline, decode.hip; the MFMA forms of rounds 1-4 are gone) at head_dim 32 and 128: several
    splits per (sequence, head) + decode_attn_combine_kernel (batch 1) and one split (batch 3), and forced split counts
    (`dec_attn_pps` 1 / 2 / 4 pages per split: another summation order each, so not bitwise equal to one another): logits within
    the kernel tolerance of the fp32 oracle, bitwise repeatable; batched == single; graph == eager."""
    cfg = LLM_CFGS[name]
    ref = {}
    for batch, ctx in ((1, 700), (3, 300)):
        eng, w = make_engine(cfg, 21, max_batch=batch, use_graph=False, max_ctx=1024, max_new=12)
        try:
            gen = torch.Generator().manual_seed(40 + batch)
            embs = [torch.randn(ctx - 17 * b, cfg["hidden_size"], generator=gen).half().float() for b in range(batch)]
            outs = {}
            for pps in (0, 0, 1, 2, 4):                      # 0 = the engine's own choice, run twice: bitwise repeatable
                if pps:
                    eng.set_option("dec_attn_pps", pps)
                eng.begin_batch(batch, 12, None)
                for b in range(batch):
                    eng.prefill(b, padded(embs[b]), embs[b].shape[0])
                logits = []
                for _ in range(6):
                    eng.decode(1)
                    logits.append(eng.logits().clone())
                cur = (eng.outputs(), torch.stack(logits))
                if pps in outs:
                    assert cur[0] == outs[pps][0] and torch.equal(cur[1], outs[pps][1])
                outs[pps] = cur
                # against the oracle: teacher-forced logits of the tokens this run produced, slot 0
                ids = cur[0][0]
                want = teacher_forced_logits(embs[0], ids[:7], w, cfg)
                got = cur[1][:, 0].float().cpu()
                observe("llm/dec_attn_split_counts_logits_max_err_over_scale", (got - want[1:7]).abs().max().item() / want.abs().max().item(), LOGIT_TOL)
            ref[batch] = (embs, outs[0])
        finally:
            eng.close()
    # graph replay == eager launches, and a batch == its sequences alone
    eng, w = make_engine(cfg, 21, max_batch=3, use_graph=True, max_ctx=1024, max_new=12)
    try:
        embs, (ids3, _) = ref[3]
        eng.begin_batch(3, 12, None)
        for b in range(3):
            eng.prefill(b, padded(embs[b]), embs[b].shape[0])
        eng.decode(6)
        assert eng.outputs() == ids3
        for b in range(3):
            assert eng.generate([padded(embs[b])], [embs[b].shape[0]], 7, eos_id=None)[0] == ids3[b]
    finally:
        eng.close()


@pytest.mark.parametrize("name,L,nseq", [("hd128", 300, 1), ("hd128", 709, 3), ("hd32", 431, 2), ("hd64", 512, 4)])
def test_pruned_last_prefill_layer_is_bitwise_the_full_one(name, L, nseq):
    """prefill_prune_last (default on): the last layer of a prefill computes K / V for every position but Q, attention, o_proj
    and the MLP for each sequence's last 128 rows only (nothing later reads the other rows: HF computes and drops them,
    modeling_llama forward -> generate keeps logits[:, -1]).  Every value that survives is produced by the same operations in
    the same order, so first-token logits, the following decode logits (which read the last layer's K / V of ALL positions)
    and the ids must be bitwise those of the unpruned layer - one sequence and a multi-sequence pass alike, and the last
    hidden rows handed back in place."""
    cfg = LLM_CFGS[name]
    eng, w = make_engine(cfg, 31, max_batch=nseq, use_graph=False, max_ctx=1024, max_new=10)
    try:
        gen = torch.Generator().manual_seed(7 * L + nseq)
        lp = (L + 31) // 32 * 32
        emb = torch.zeros(nseq, lp, cfg["hidden_size"], dtype=torch.float16, device="cuda")
        emb[:, :L] = (torch.randn(nseq, L, cfg["hidden_size"], generator=gen)).half().cuda()
        outs = {}
        for prune in (0, 1):
            eng.set_option("prefill_prune_last", prune)
            eng.begin_batch(nseq, 10, None)
            x = emb.clone()
            if nseq == 1:
                eng.prefill(0, x[0], L)
            else:
                eng.prefill_batch(0, nseq, x.view(nseq * lp, -1), L)
            first = eng.logits().clone()
            logits = []
            for _ in range(5):
                eng.decode(1)
                logits.append(eng.logits().clone())
            torch.cuda.synchronize()
            outs[prune] = (first, torch.stack(logits), eng.outputs(), x[:, L - 1].clone(), x[:, : lp - 128].clone())
        assert torch.equal(outs[0][0], outs[1][0])
        assert torch.equal(outs[0][1], outs[1][1])
        assert outs[0][2] == outs[1][2]
        assert torch.equal(outs[0][3], outs[1][3])           # the last position's final hidden state, in place
        assert not torch.equal(outs[0][4], outs[1][4])       # ... and the pruning really happened: the other rows stop one layer early
    finally:
        eng.set_option("prefill_prune_last", 1)
        eng.close()




@pytest.mark.parametrize("batch,pps", [(8, 0), (8, 4), (12, 0)])
def test_workgroup_local_attention_splits_are_bitwise_the_combine_kernel(batch, pps):
    """Round 5: engines of 8-15 slots x 32 heads give the decode attention one workgroup per CU and still split every context in 2 (or 4);
    the splits of a (sequence, head) are then the WAVES of one workgroup, joined through LDS behind a barrier instead of through global
    partials and decode_attn_combine_kernel.  Same operations in the same order: ids and logits bit for bit against `dec_attn_local` 0,
    ragged contexts (a split with no page of its own included), eager and as a hipGraph."""
    cfg = dict(LLM_CFGS["hd128"], num_attention_heads=32, hidden_size=4096, intermediate_size=512, num_hidden_layers=1)
    gen = torch.Generator().manual_seed(700 + batch)
    lens = [700 - 41 * b for b in range(batch)]
    embs = [(torch.randn(L, cfg["hidden_size"], generator=gen) * 0.5).half().float() for L in lens]
    res = {}
    for use_graph in (False, True):
        eng, w = make_engine(cfg, 29, max_batch=batch, use_graph=use_graph, max_ctx=1024, max_new=12)
        try:
            for local in (1, 0, 1):
                eng.set_option("dec_attn_local", local)
                if pps:
                    eng.set_option("dec_attn_pps", pps)
                eng.begin_batch(batch, 12, None)
                for b in range(batch):
                    eng.prefill(b, padded(embs[b]), lens[b])
                logits = []
                for _ in range(6):
                    eng.decode(1)
                    logits.append(eng.logits().clone())
                cur = (eng.outputs(), torch.stack(logits))
                if (use_graph, local) in res:
                    assert cur[0] == res[(use_graph, local)][0] and torch.equal(cur[1], res[(use_graph, local)][1])
                res[(use_graph, local)] = cur
        finally:
            eng.close()
    base = res[(False, 0)]
    for key, cur in res.items():
        assert cur[0] == base[0], key
        assert torch.equal(cur[1], base[1]), key

"""The attention record through the decode path (`attn_map=`): three prompts of 60, 64 and 70 tokens, so that the decode crosses a page
edge, 8 new tokens, a window of 128 keys.  The ids do not change; captured step == eager step, batch of 3 == alone, either bank, all
bitwise; row 0 and rows at or beyond the length are zeros and every recorded row sums to 1; against an fp64 restatement of the small
Llama (tests/attn_map_ref.py), teacher-forced with the generated ids; finished slots, slot_reset, continuous batching, the device
collect, a single layer against the all-layer mean, the `llm.generate` seam, the ABI.

Against fp64 no tolerance is fixed: each row may differ by the kernel bound (tests/attn_map_ref.py derived_bound) plus twice the error
the same map shows when that restatement rounds to fp16 wherever the engine holds fp16 (two fp16 paths round differently, and the
sample is small).  Seen on an MI355X (test_against_fp64 prints them) - largest |engine - fp64|, the fp16 restatement's own largest
error, worst error / allowance: hd32 4.04e-6, 3.40e-6, 0.054; hd64 1.21e-5, 1.22e-5, 0.057; hd128 2.19e-5, 1.88e-5, 0.064."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.attn_map_ref import teacher_forced_maps
from tests.test_gpu_llm import LLM_CFGS, make_engine, padded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS, NEW, W = (60, 64, 70), 8, 128
AM = dict(keys=W)


def prompts(cfg, lens=LENS, seed=31):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(L, cfg["hidden_size"], generator=gen).half().float() for L in lens]


def check_record(r, L):
    """shape, zeros where nothing is recorded, rows that sum to 1 (the window covers the context)"""
    a, n = r["attn_map"], len(r["ids"])
    assert a.dtype == np.float32 and a.shape == (n, W)
    assert not a[0].any()
    for i in range(1, n):
        npos = L + i
        assert not a[i, npos:].any() and (a[i, :npos] >= 0).all()
        assert abs(float(a[i].astype(np.float64).sum()) - 1.0) <= npos * 2.0 ** -22, (i, float(a[i].astype(np.float64).sum()))


def same(a, b):
    return a["ids"] == b["ids"] and a["attn_map"].shape == b["attn_map"].shape and a["attn_map"].tobytes() == b["attn_map"].tobytes()


@pytest.fixture(scope="module")
def eng3():
    """hd32, three slots, captured decode step; `plain`: the ids BEFORE anything asked for a map"""
    cfg = LLM_CFGS["hd32"]
    e, w = make_engine(cfg, 5, max_batch=3, use_graph=True, max_new=NEW)
    base = prompts(cfg)
    embs = lambda: [padded(x) for x in base]                      # a prefill clobbers its embeddings: fresh copies for every use
    plain = e.generate(embs(), LENS, NEW, eos_id=None)
    assert not e._am_on and not e._am_bufs                        # a process that never asks allocates nothing
    yield e, cfg, w, base, embs, plain
    e.close()


def test_the_ids_do_not_change_and_the_rows_are_distributions(eng3):
    eng, cfg, w, base, embs, plain = eng3
    got = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM)
    assert [r["ids"] for r in got] == plain and all(len(p) == NEW for p in plain)
    for r, L in zip(got, LENS):
        check_record(r, L)
    both = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM, logprobs=2)
    assert [same(a, b) for a, b in zip(both, got)] == [True] * 3 and "token_logprobs" in both[0]
    auto = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=dict(keys=None))       # the longest prompt rounded up to 64: 128
    assert [same(a, b) for a, b in zip(auto, got)] == [True] * 3


def test_a_sequence_in_a_batch_of_3_gets_what_it_gets_alone(eng3):
    eng, cfg, w, base, embs, plain = eng3
    together = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM)
    for b in range(3):
        assert same(eng.generate([embs()[b]], [LENS[b]], NEW, eos_id=None, attn_map=AM)[0], together[b]), b


@pytest.mark.parametrize("name", list(LLM_CFGS))
def test_captured_eager_and_either_bank_give_the_same_bits(name):
    cfg = LLM_CFGS[name]
    base = prompts(cfg)
    outs = []
    for use_graph, bank in ((False, 0), (True, 0), (True, 1)):
        from aurora_amd.engine import AuroraCapEngine
        from tests.util import rand_llm_weights
        eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 5)}, max_frames=1, max_batch=3, max_ctx=512,
                              max_new_tokens=NEW, use_graph=use_graph, num_banks=2)
        try:
            eng.select_bank(bank)
            plain = eng.generate([padded(x) for x in base], LENS, NEW, eos_id=None)
            outs.append(eng.generate([padded(x) for x in base], LENS, NEW, eos_id=None, attn_map=AM))
            assert [r["ids"] for r in outs[-1]] == plain
            assert sorted(eng._am_on) == [bank]
        finally:
            eng.close()
    for o in outs[1:]:
        assert [same(a, b) for a, b in zip(o, outs[0])] == [True] * 3


@pytest.mark.parametrize("name", list(LLM_CFGS))
def test_against_fp64(name):
    """Measured on an MI355X, the fp16 restatement's largest error against fp64 over the three captions (the allowance is twice that
    plus the kernel bound): hd32 3.40e-6, hd64 1.22e-5, hd128 1.88e-5; the engine's own 4.04e-6, 1.21e-5, 2.19e-5; worst error /
    allowance 0.054, 0.057, 0.064."""
    cfg = LLM_CFGS[name]
    eng, w = make_engine(cfg, 5, max_batch=3, use_graph=True, max_new=NEW)
    try:
        base = prompts(cfg)
        got = eng.generate([padded(x) for x in base], LENS, NEW, eos_id=None, attn_map=AM)
    finally:
        eng.close()
    f16 = lambda t: t.half().to(t.dtype)
    worst, e_gpu, e_f16 = 0.0, 0.0, 0.0
    for r, emb in zip(got, base):
        ref, bound = teacher_forced_maps(emb, r["ids"], w, cfg, W)
        half, _ = teacher_forced_maps(emb, r["ids"], w, cfg, W, quant=f16)
        err16 = float((half - ref).abs().max())
        allow = 2.0 * err16 + bound
        diff = (torch.from_numpy(r["attn_map"]).double() - ref).abs()
        worst, e_gpu, e_f16 = max(worst, float((diff / allow).max())), max(e_gpu, float(diff.max())), max(e_f16, err16)
    print(f"attention map {name} against fp64: largest |engine - fp64| {e_gpu:.3e}, the fp16 restatement's {e_f16:.3e}, "
          f"worst error / allowance {worst:.3f}")
    assert worst <= 1.0


def test_a_single_layer_and_the_mean_taken_by_hand(eng3):
    eng, cfg, w, base, embs, plain = eng3
    one = [eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=dict(keys=W, layers=[l])) for l in (0, 1)]
    last = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=dict(keys=W, layers=[-1]))
    assert [same(a, b) for a, b in zip(last, one[1])] == [True] * 3
    both = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=dict(keys=W, layers=[0, 1]))
    allof = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM)
    assert [same(a, b) for a, b in zip(both, allof)] == [True] * 3                      # the model has two layers
    for b in range(3):
        assert one[0][b]["ids"] == plain[b] and not np.array_equal(one[0][b]["attn_map"], one[1][b]["attn_map"])
        # each single-layer record is (sum over heads) * fp32(1/4), the two-layer record (sum0 * fp32(1/8)) + (sum1 * fp32(1/8)): powers of
        # two, so halving is exact and the only rounding left is the one addition
        hand = one[0][b]["attn_map"] * np.float32(0.5) + one[1][b]["attn_map"] * np.float32(0.5)
        assert hand.tobytes() == allof[b]["attn_map"].tobytes(), b
    refs = [teacher_forced_maps(base[0], plain[0], w, cfg, W, layers=[l])[0] for l in (0, 1)]
    dist = lambda r, ref: float((torch.from_numpy(r["attn_map"]).double() - ref).abs().max())      # noqa: E731
    for l in (0, 1):                                              # bit l of the mask is layer l, not its neighbour
        assert dist(one[l][0], refs[l]) < 0.1 * dist(one[l][0], refs[1 - l]), l


def test_a_finished_slot_stops_recording(eng3):
    eng, cfg, w, base, embs, plain = eng3
    eos = plain[1][3]
    want = [p[: p.index(eos) + 1] if eos in p else p for p in plain]
    assert len(want[1]) <= 4
    full = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM)
    got = eng.generate(embs(), LENS, NEW, eos_id=eos, attn_map=AM, check_every=NEW)      # the finished slot sits through the later steps
    assert [r["ids"] for r in got] == want
    state = eng.attn_map_state()
    for b in range(3):
        n = len(want[b])
        assert got[b]["attn_map"].tobytes() == full[b]["attn_map"][:n].tobytes()
        assert not state[b, n:].any(), "rows at or beyond the length must stay zero"


def test_slot_reset_clears_the_rows_and_a_refill_records_from_row_1(eng3):
    eng, cfg, w, base, embs, plain = eng3
    alone = eng.generate([embs()[2]], [LENS[2]], NEW, eos_id=None, attn_map=AM)[0]
    e = embs()
    eng.begin_batch(2, NEW, None)
    eng.prefill(0, e[0], LENS[0])
    eng.prefill(1, e[1], LENS[1])
    eng.decode(3)
    before = eng.attn_map_state()
    assert before[0, 1:4].any() and before[1, 1:4].any() and not before[:, 4:].any() and not before[:, 0].any()
    eng.slot_reset(0)
    cleared = eng.attn_map_state()
    assert not cleared[0].any() and cleared[1].tobytes() == before[1].tobytes()
    eng.prefill(0, e[2], LENS[2])
    eng.decode(2)
    after = eng.attn_map_state()
    assert not after[0, 0].any() and not after[0, 3:].any()
    assert after[0, :3].tobytes() == alone["attn_map"][:3].tobytes()
    assert after[1, :4].tobytes() == before[1, :4].tobytes() and after[1, 4:6].any() and not after[1, 6:].any()


def test_slot_collect_attn_map_equals_the_state(eng3):
    eng, cfg, w, base, embs, plain = eng3
    got = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM)
    out = torch.full((2, NEW, W), -1.0, dtype=torch.float32, device="cuda")
    eng.slot_collect_attn_map(1, 2, out)
    torch.cuda.synchronize()
    state = eng.attn_map_state()
    assert out.cpu().numpy().tobytes() == state[1:3].tobytes()
    assert state[1].tobytes() == got[1]["attn_map"].tobytes()


def test_off_after_on_launches_nothing_and_leaves_the_buffer_alone(eng3):
    eng, cfg, w, base, embs, plain = eng3
    on = eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM)
    buf = eng._am_bufs[eng._bank]
    eng.attn_map_off()
    assert not eng._am_on
    torch.cuda.synchronize()
    buf.fill_(0xA5)
    assert eng.generate(embs(), LENS, NEW, eos_id=None) == plain
    eng.slot_reset(1)
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), "a bank that no longer records wrote its old buffer"
    assert [same(a, b) for a, b in zip(eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=AM), on)] == [True] * 3      # and on again


def test_enable_is_refused_inside_a_capture_and_for_bad_arguments(eng3):
    from aurora_amd._lib import AuroraHipError
    eng, cfg, w, base, embs, plain = eng3
    with pytest.raises(ValueError):
        eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=dict(keys=100))
    with pytest.raises(ValueError):
        eng.generate(embs(), LENS, NEW, eos_id=None, attn_map=dict(keys=64, layers=[2]))
    with pytest.raises(ValueError):
        eng._attn_map_on(1024)                                        # beyond the engine's context of 512
    buf = torch.empty(int(eng.L.aur_attn_map_bytes(eng.ctx, 64)), dtype=torch.uint8, device="cuda")
    rc = eng.L.aur_attn_map_enable(eng.ctx, 64, 0, buf.data_ptr(), buf.numel() - 1, None)
    assert rc == -1                                                   # AUR_ERR_ARG: a buffer one byte short
    rc = eng.L.aur_attn_map_enable(eng.ctx, 64, 1 << 5, buf.data_ptr(), buf.numel(), None)
    assert rc == -1                                                   # layer 5 of a two-layer model
    from aurora_amd._lib import check
    eng.begin_batch(1, NEW, None)
    with pytest.raises(AuroraHipError, match="status -2"):            # AUR_ERR_STATE, before the runtime is touched
        eng.graph_capture(lambda: check(eng.ctx, eng.L.aur_attn_map_enable(eng.ctx, 64, 0, buf.data_ptr(), buf.numel(), eng._stream()),
                                        "aur_attn_map_enable"))
    torch.cuda.synchronize()
    assert eng.generate(embs(), LENS, NEW, eos_id=None) == plain


# ------------------------------------------------------------------------------------------------ the whole path (tiny ViT + projector + Llama)
def whole_path_engine(max_batch, max_new, spare=0, max_frames=4):
    from aurora_amd.engine import AuroraCapEngine
    from tests.test_gpu_caption_batch import VCFG, weights
    return AuroraCapEngine({"vit": VCFG, "llm": LLM_CFGS["hd32"]}, weights(), max_frames=max_frames, max_batch=max_batch, max_ctx=512,
                           max_new_tokens=max_new, spare_slots=spare)


@pytest.mark.parametrize("spare", [0, 2])
def test_continuous_batching_gives_every_clip_the_map_it_gets_alone(spare):
    """7 ragged clips through 3 slots with EOS stopping, so that slots are refilled: spare = 0 is the plain schedule (overlap=False),
    spare = 2 the overlapped one (front ends staged beside the decode, committed into freed slots)"""
    from tests.test_gpu_caption_batch import clips
    eng = whole_path_engine(3, NEW, spare)
    try:
        cs = clips(7, 9)
        free = [eng.caption_ids(px, ids, 0.5, NEW, eos_id=None) for px, ids in cs]
        eos = free[2][5]
        am = dict(keys=256)
        want = [eng.caption_ids(px, ids, 0.5, NEW, eos_id=eos, attn_map=am) for px, ids in cs]
        assert [x["ids"] for x in want] == [a[: a.index(eos) + 1] if eos in a else a for a in free]
        assert len({len(x["ids"]) for x in want}) > 1 and all(x["attn_map"][1:].any() for x in want if len(x["ids"]) > 1)
        got = dict(eng.caption_stream(cs, 0.5, NEW, eos_id=eos, check_every=4, attn_map=am, **({} if spare else dict(overlap=False))))
        assert sorted(got) == list(range(7))
        for i in range(7):
            assert same(got[i], want[i]), i
        batch = eng.caption_batch(cs[:3], 0.5, NEW, eos_id=eos, attn_map=am)
        assert [same(a, b) for a, b in zip(batch, want[:3])] == [True] * 3
    finally:
        eng.close()


def test_the_generate_seam_and_the_visual_columns():
    from aurora_amd import attn_map as A
    from aurora_amd.model import AuroraModel, GenerateOutput
    from tests.test_gpu_loglikelihood import IDS
    eng = whole_path_engine(1, NEW, max_frames=3)
    try:
        m = AuroraModel(eng, eos_token_id=None)
        m.visual_encoder.reset_tome_r(0.5)
        px = torch.randn(3, 3, 56, 56, generator=torch.Generator().manual_seed(76)).half()
        out = m({"pixel_values": px.unsqueeze(0), "input_ids": torch.tensor([IDS]), "output_attentions": True}, mode="inference")
        rows = out["vis_rows"]
        assert rows.dtype == torch.int32 and rows.numel() > 0 and int(rows.max()) < out["inputs_embeds"].shape[1]
        plain = m.llm.generate(**out, do_sample=False, max_new_tokens=NEW)
        assert torch.is_tensor(plain) and plain.shape == (1, NEW)
        with pytest.raises(ValueError):
            m.llm.generate(**out, max_new_tokens=NEW, output_attentions=True)
        r = m.llm.generate(**out, do_sample=False, max_new_tokens=NEW, return_dict_in_generate=True, output_attentions=True)
        Wd = A.window_for(out["inputs_embeds"].shape[1])
        assert isinstance(r, GenerateOutput) and torch.equal(r.sequences, plain) and r.token_logprobs is None
        assert r.prompt_attention.shape == (1, NEW, Wd) and r.prompt_attention.dtype == torch.float32
        assert r.visual_attention.shape == (NEW, rows.numel()) and r.visual_share.shape == (NEW,)
        assert torch.equal(r.visual_attention, r.prompt_attention[0][:, rows.long()])
        assert float(r.visual_share[0]) == 0.0 and bool((r.visual_share[1:] > 0).all()) and bool((r.visual_share <= 1.0 + 1e-6).all())
        bare = m.llm.generate(**out, do_sample=False, max_new_tokens=NEW, return_dict_in_generate=True)
        assert torch.equal(bare.sequences, plain) and bare.prompt_attention is None
        got = m.caption_batch([(px, IDS)], max_new_tokens=NEW, attn_map=dict(keys=None))[0]
        assert got["ids"] == plain[0].tolist() and got["attn_map"].tobytes() == r.prompt_attention[0].numpy().tobytes()
        assert got["visual_share"].tobytes() == r.visual_share.numpy().tobytes()
    finally:
        eng.close()


def test_cli_writes_a_heat_map_per_generated_token(tmp_path):
    import subprocess
    import sys
    m, a, png = (str(tmp_path / n) for n in ("m.npz", "a.npz", "a.png"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--synthetic", "--merge_map", m, "--attn_map", a, "--attn_vis", png,
                          "--max_new_tokens", "4", "--num_frm", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    ids = [int(x) for x in out.stdout.strip().split("\n")[-1].strip("[]").split(",")]
    rec, mm = np.load(a), np.load(m)
    assert rec["ids"].tolist() == ids and len(ids) == 4
    n, nvis = rec["visual_attention"].shape
    assert n == 4 and nvis == int(mm["n_kept"].sum()) == len(rec["vis_rows"]) and rec["attn_map"].shape[0] == 4
    assert not rec["attn_map"][0].any() and np.allclose(rec["attn_map"][1:].sum(1), 1.0, atol=1e-3)
    assert np.array_equal(rec["visual_share"], rec["visual_attention"].sum(1, dtype=np.float32)) and (rec["visual_share"][1:] > 0).all()
    from PIL import Image
    img = np.asarray(Image.open(png))
    frames, gh, gw = mm["merge_map"].shape
    patch = max(1, 112 // gw)
    assert img.shape == (4 * (gh * patch + 1) - 1, frames * (gw * patch + 1) - 1, 3)
    assert not img[: gh * patch, : gw * patch].any() and img[gh * patch + 1: 2 * gh * patch + 1].max() == 255      # token 0 has no record


def test_the_new_exports_are_in_the_library():
    from aurora_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aurora_hip.h")).read()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ("aur_attn_map_bytes", "aur_attn_map_enable", "aur_get_attn_map", "aur_slot_collect_attn_map", "aur_attn_map_rows_scratch_bytes",
                 "aur_attn_map_rows"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and f"{name}(" in hdr, name

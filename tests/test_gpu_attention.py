"""The two attention kernels alone - attn_kernel<KBLK, VD16> (attn.hip: ViT and causal prefill, every instantiation) and
decode_attn_dot_kernel + decode_attn_combine_kernel (decode.hip) - against the fp64 definition, elementwise, under the bound derived
from their stated arithmetic (tests/attn_ref.py derived_bound; nothing here is an observed tolerance).  The kernels are reached through
aur_attn_rows / aur_attn_decode_rows: the layer's own QKV epilogue with the identity as weight writes exactly the caller's q, k, v into
the fragments, then the production attention launch runs.  tests/test_attention_reference.py shows on the CPU that an off-by-one mask,
a missing newest key, a stale page, a mishandled empty split or a missing rescale leaves this bound by more than 100x at every shape.

Worst error / bound seen on an MI355X: attn_kernel 0.92 (by value), 0.83 (device lengths), 0.20 (RoPE); decode kernels 0.78 (six
splits and fewer), 0.61 (18 splits), 0.21 (RoPE).  Each test prints its own."""
import pytest
import torch

from tests.attn_ref import (DEC_CASES, DEC_POS, FLASH_CASES, attention_fp64, build_case, derived_bound, flash_shapes, rope_apply, rope_delta, rup,
                            visible, worst_ratio)
from tests.test_gpu_llm import LLM_CFGS
from tests.util import rand_llm_weights

pytestmark = pytest.mark.gpu

# token capacity 14 x 14 + 1 = 197 (224 padded rows): four key blocks, two query workgroups.  hd 80 is the <3, 5> instantiation (K padded to 96)
VIT_CFGS = {
    "vit_hd16": dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=2, intermediate_size=64, patch_size=14, image_size=196,
                     hidden_act="quick_gelu"),
    "vit_hd80": dict(hidden_size=320, num_attention_heads=4, num_hidden_layers=2, intermediate_size=320, patch_size=14, image_size=196,
                     hidden_act="quick_gelu"),
}
CFGS = list(VIT_CFGS) + list(LLM_CFGS)
SLOTS, CTX, CTX_BIG = 16, 384, 1152         # decode engines: 16 slots of 6 pages; one of 18 pages (the combine's generic loop)
_ENGINES = {}


def engine(name):
    """one engine per config for the whole module: (engine, layout, heads, hd, packed identity, RoPE settings)"""
    if name not in _ENGINES:
        from aurora_amd.engine import AuroraCapEngine
        if name in VIT_CFGS:
            cfg, layout = VIT_CFGS[name], "vit"
            eng = AuroraCapEngine({"vit": cfg, "llm": None}, {}, max_frames=4, max_batch=1, max_ctx=64, max_new_tokens=8, use_graph=False)
        else:
            cfg, layout = LLM_CFGS[name.split("@")[0]], "llm"
            eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 3)}, max_frames=1, max_batch=SLOTS,
                                  max_ctx=CTX_BIG if name.endswith("@big") else CTX, max_new_tokens=8, use_graph=False)
        heads = cfg["num_attention_heads"]
        rope = dict(theta=cfg.get("rope_theta", 1e4), factor=cfg.get("rope_factor", 1.0))
        _ENGINES[name] = (eng, layout, heads, cfg["hidden_size"] // heads, eng.attn_identity_weight(layout), rope)
    return _ENGINES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e[0].close()
    _ENGINES.clear()


def stack_cases(name, hd, n_valids, rows, heads, seed, rope_safe=False):
    """q, k, v [nseq, heads, rows, hd]: one independent case per (sequence, head); sequence i has n_valids[i] valid rows"""
    qkv = [[build_case(name, hd, n, rows, seed * 1000 + i * 16 + h, rope_safe) for h in range(heads)] for i, n in enumerate(n_valids)]
    return tuple(torch.stack([torch.stack([qkv[i][h][j] for h in range(heads)]) for i in range(len(n_valids))]) for j in range(3))


def as_rows(q, k, v):
    """[nseq, heads, rows, hd] x 3 -> x [nseq * rows, 3 * heads * hd] = [q | k | v], heads side by side"""
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0] * t.shape[2], -1)
    return torch.cat([flat(q), flat(k), flat(v)], 1)


def as_heads(out, nseq, rows, heads, hd):
    return out.float().cpu().view(nseq, rows, heads, hd).permute(0, 2, 1, 3)


def reference(q, k, v, n_valid, causal, rope=None, q_rows=None):
    """fp64 reference and bound for queries q_rows (default: the valid rows) of one stack [.., rows, hd] whose sequences share n_valid"""
    hd, rows = q.shape[-1], k.shape[-2]
    q_rows = q_rows if q_rows is not None else slice(0, n_valid)
    q_pos0 = q_rows.start
    delta = 0.0
    if rope:
        pos = torch.arange(rows)
        q, k = rope_apply(q, pos, **rope), rope_apply(k, pos, **rope)
        delta = rope_delta(q[..., q_rows, :], k, hd ** -0.5, visible(q_rows.stop - q_rows.start, rows, causal, n_valid, q_pos0))
    return attention_fp64(q[..., q_rows, :], k, v, hd ** -0.5, causal, n_valid, q_pos0), delta


# ------------------------------------------------------------------------------------------------------------ attn_kernel
# (causal, case): the future construction needs the causal mask
MODES = [pytest.param(causal, case, id=f"{'causal' if causal else 'full'}-{case}") for causal in (False, True) for case in FLASH_CASES
         if causal or case != "future"]


@pytest.mark.parametrize("causal,case", MODES)
@pytest.mark.parametrize("name", CFGS)
def test_prefill_attention_by_value(name, causal, case):
    """every n_valid each side of the 16-key tile, the 32-row wave, the 64-key block and the 128-row workgroup; 3 sequences x 4 heads
    (2 at hd 128): 12 pairs on the padded XCD grid map.  Rows at or beyond n_valid are poison and are not compared."""
    eng, layout, heads, hd, w, _ = engine(name)
    worst, at = 0.0, None
    for n_valid, rows in flash_shapes():
        q, k, v = stack_cases(case, hd, [n_valid] * 3, rows, heads, n_valid * 7 + rows)
        out = as_heads(eng.attn_rows(as_rows(q, k, v), w, layout=layout, nseq=3, rows=rows, causal=causal, t=n_valid), 3, rows, heads, hd)
        assert torch.isfinite(out).all(), (n_valid, rows)
        ref, delta = reference(q, k, v, n_valid, causal)
        r = worst_ratio(out[..., :n_valid, :], ref.o, derived_bound(ref, 1, delta))
        if r > worst:
            worst, at = r, (n_valid, rows)
    print(f"attn_kernel {name} {'causal' if causal else 'full'} {case}: worst error / bound {worst:.3f} at (n_valid, rows) {at}")
    assert worst <= 1.0, (worst, at)


@pytest.mark.parametrize("case", FLASH_CASES)
@pytest.mark.parametrize("name", CFGS)
def test_prefill_attention_with_device_lengths(name, case):
    """four sequences of different lengths in one launch, the lengths in device memory: {1, 65, 128, stride} (a whole padding query
    block, a length that ends a block, a full sequence) and {97, 128, 65, 111} at stride 128.  Output rows at or beyond a sequence's
    length are exactly zero (the kernel's contract); rows [len, stride) of the input are poison."""
    eng, layout, heads, hd, w, _ = engine(name)
    worst = 0.0
    for lens, stride in (([1, 65, 128, 160], 160), ([97, 128, 65, 111], 128)):
        q, k, v = stack_cases(case, hd, lens, stride, heads, stride + 3)
        out = as_heads(eng.attn_rows(as_rows(q, k, v), w, layout=layout, nseq=4, rows=stride, causal=True, lens=lens), 4, stride, heads, hd)
        assert torch.isfinite(out).all()
        for i, n in enumerate(lens):
            assert not out[i, :, n:].any(), (lens, i, "rows at or beyond the length must be zero")
            ref, delta = reference(q[i], k[i], v[i], n, True)
            worst = max(worst, worst_ratio(out[i, :, :n], ref.o, derived_bound(ref, 1, delta)))
    print(f"attn_kernel {name} device lengths {case}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(LLM_CFGS))
def test_prefill_attention_with_rope(name):
    """RoPE on (the epilogue's table rotation, then fp16): rand inputs with |q||k| scale <= 2, positions across the 64-token pages"""
    eng, layout, heads, hd, w, rope = engine(name)
    worst = 0.0
    for n_valid, rows in ((65, 96), (129, 160), (193, 224)):
        q, k, v = stack_cases("rand", hd, [n_valid] * 3, rows, heads, n_valid, rope_safe=True)
        out = as_heads(eng.attn_rows(as_rows(q, k, v), w, layout=layout, nseq=3, rows=rows, causal=True, t=n_valid, rope=True), 3, rows, heads, hd)
        assert torch.isfinite(out).all()
        ref, delta = reference(q, k, v, n_valid, True, rope)
        assert delta <= 2.0 ** -9
        worst = max(worst, worst_ratio(out[..., :n_valid, :], ref.o, derived_bound(ref, 1, delta)))
    print(f"attn_kernel {name} rope: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_attention_entry_points_reject_bad_arguments():
    from aurora_amd._lib import AuroraHipError
    eng, layout, heads, hd, w, _ = engine("hd32")
    x = torch.zeros(64, 3 * heads * hd)
    for kw in (dict(nseq=1, rows=64, t=65), dict(nseq=1, rows=64, t=0), dict(nseq=SLOTS + 1, rows=32, t=1), dict(nseq=1, rows=48, t=1),
               dict(nseq=1, rows=CTX + 32, t=1), dict(nseq=1, rows=64, t=1, seq0=SLOTS)):
        xx = torch.zeros(kw["nseq"] * kw["rows"], 3 * heads * hd)
        with pytest.raises(AuroraHipError, match="status -1"):
            eng.attn_rows(xx, w, layout=layout, causal=True, **kw)
    with pytest.raises(AuroraHipError, match="status -1"):
        eng.attn_rows(x[:, :-32], w, layout=layout, nseq=1, rows=64, causal=True, t=1)               # kx not a multiple of 64
    with pytest.raises(AuroraHipError, match="status -1"):
        eng.attn_decode_rows(torch.zeros(SLOTS + 1, 3 * heads * hd), w, [0] * (SLOTS + 1))
    assert torch.isfinite(eng.attn_rows(x, w, layout=layout, nseq=1, rows=64, causal=True, t=64).float()).all()      # the ctx is still usable


# ------------------------------------------------------------------------------------------------------------ decode kernels
def decode_case(name, case, ctx, rope_on, pps_list):
    """Fill the pages of the 16 sequences through the prefill entry - valid K / V at [0, pos_b), poison from pos_b to the end of the
    context, whole later pages included - then one ragged decode step per split geometry: the step writes its own K / V at pos_b.
    Returns the worst error / bound.  Every result must repeat bitwise."""
    eng, layout, heads, hd, w, rope = engine(name)
    rope = rope if rope_on else None
    pos = list(DEC_POS)
    q, k, v = stack_cases(case, hd, [p + 1 for p in pos], ctx, heads, 77 + ctx, rope_safe=rope_on)
    kf, vf = k.clone(), v.clone()
    for b, p in enumerate(pos):             # the cache before the step: position pos_b is still poison
        kf[b, :, p], vf[b, :, p] = k[b, :, p + 1], v[b, :, p + 1]
    eng.attn_rows(as_rows(q, kf, vf), w, layout=layout, nseq=SLOTS, rows=ctx, causal=True, t=ctx, rope=rope_on)
    idx = torch.tensor(pos)
    step = lambda t: t[torch.arange(SLOTS), :, idx].reshape(SLOTS, heads * hd)          # row pos_b of every (sequence, head)
    x = torch.cat([step(q), step(k), step(v)], 1)
    refs = []
    for b, p in enumerate(pos):
        refs.append(reference(q[b], k[b], v[b], p + 1, False, rope, q_rows=slice(p, p + 1)))
    worst = 0.0
    pages = ctx // 64
    for pps in pps_list:
        eng.set_option("dec_attn_pps", pps)
        out = eng.attn_decode_rows(x, w, pos, rope=rope_on)
        assert torch.equal(out, eng.attn_decode_rows(x, w, pos, rope=rope_on)), ("not repeatable", pps)
        out = out.float().cpu().view(SLOTS, heads, 1, hd)
        assert torch.isfinite(out).all(), pps
        nsplit = (pages + pps - 1) // pps
        for b in range(SLOTS):
            ref, delta = refs[b]
            r = worst_ratio(out[b], ref.o, derived_bound(ref, nsplit, delta))
            assert r <= 1.0, (case, "pps", pps, "pos", pos[b], r)
            worst = max(worst, r)
    return worst


def default_pps(heads, pages):
    """the split geometry aur_create derives from the capacity (engine.hip derive): enough splits for ~512 waves, at most 16"""
    want = min(max((512 + heads * SLOTS - 1) // (heads * SLOTS), 1), 16)
    return max((pages + want - 1) // want, 1)


@pytest.mark.parametrize("case", DEC_CASES + ("rand+rope",))
@pytest.mark.parametrize("name", list(LLM_CFGS))
def test_decode_attention(name, case):
    """one ragged launch, pos each side of the 16-token fragment row and the 64-token page up to five pages; pages per split: the
    engine's default, 1, 2, 4 and beyond the context (a single split: the kernel normalises and stores itself)"""
    heads = LLM_CFGS[name]["num_attention_heads"]
    dflt = default_pps(heads, CTX // 64)
    try:
        worst = decode_case(name, case.split("+")[0], CTX, "+rope" in case, [dflt, 1, 2, 4, 64])
    finally:
        engine(name)[0].set_option("dec_attn_pps", dflt)
    print(f"decode attention {name} {case}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("case", DEC_CASES)
def test_decode_attention_with_eighteen_splits(case):
    """an engine of 1152 positions at one page per split: 18 splits, the combine's generic loop instead of its <= 16 form; most splits
    are empty for most sequences"""
    worst = decode_case("hd64@big", case, CTX_BIG, False, [1])
    print(f"decode attention hd64, 18 splits, {case}: worst error / bound {worst:.3f}")

"""GPU parity under trained-checkpoint statistics (tests/util.py `ckpt_like_*`), through the C ABI.

Every other floating-point comparison of this suite feeds the kernels N(0, sigma^2) data and holds them to bounds calibrated from their
own output.  Here the data has what a trained Vicuna / CLIP ViT-H has - RMSNorm weights from 0.001 to 16, a residual stream with
persistent outlier channels and a massive first row, heavy-tailed matrices, sharp attention - and the bound does NOT come from the
kernels: tests/golden/g17_ckpt_stats.npz records how far the reference's own arithmetic (HF Llama / the reference's encoder layer,
`torch.float16`) is from an fp64 evaluation of the same inputs, and the HIP path may be at most 1.5x as far (1.5, not 1: HF fp16 on a
CPU is not bit-identical to HF fp16 on a GPU, and a CPU emulation of this project's arithmetic sat at 0.6 - 0.9 of it; one extra fp16
rounding of the residual stream would not fit).  No entry of tests/parity_bounds.PER_COMPARISON belongs to these keys.

Three design choices are what this exercises: norm weights folded into the consuming projection in fp16 (engine.py `fold`: with
w_norm ~ 0.03 part of W' is below fp16's normal range), sum(x^2) carried as 2^-28 fixed point in 64-bit integers by the decode step
(decode.hip; embed scales 2^-10 .. 2^6: from partials that round to a handful of units up to 1e17, past fp32's integer range), and the
exp2-form softmax with P rounded to fp16 (attn.hip, decode.hip; a sink row, logit gains 3 and 8, 1 / 3 / 5-page splits).
Kernel-level companions below: the norm kernels and the GEMMs against fp64 with bounds derived from their summation structure, and
the greedy pick on exact ties.
"""
import numpy as np
import pytest
import torch

from oracle import aurora_oracle as O
from oracle import tome_ref
from tests.test_gpu_llm import LLM_CFGS, LLM_CFGS_VOCAB, padded
from tests.util import (CKPT_LLM_CFG, CKPT_NEW_TOKENS, CKPT_VIT_CASES, ckpt_like_llm_case, ckpt_like_vit_input, ckpt_like_vit_weights,
                        ckpt_llm_cases, gemm_bound, golden, observe, outlier_operands, rand_llm_weights, rel_l2, to_match, tt)

pytestmark = pytest.mark.gpu

MARGIN = 1.5
NEW = CKPT_NEW_TOKENS


def combos():
    """the cases grouped by what shares one set of weights: {(seed, gain, scale): [(name, T)]}"""
    out = {}
    for name, seed, gain, scale, T in ckpt_llm_cases():
        out.setdefault((seed, gain, scale), []).append((name, T))
    return out


COMBOS = combos()
COMBO_IDS = [f"s{s}_g{int(g)}_e{int(np.log2(sc))}" for s, g, sc in COMBOS]


class Case:
    """one fixture case: inputs regenerated from the seeds (their sha256 is pinned by tests/test_oracle_golden.py), fp64 logits at
    the stored rows, the per-row HF-fp16 error.  Row T - 1 + j predicts new token j."""

    def __init__(self, name, seed, gain, scale, T):
        g = golden("g17_ckpt_stats.npz")
        p = f"llm.{name}."
        self.name, self.T = name, T
        self.w, self.emb = ckpt_like_llm_case(CKPT_LLM_CFG, seed, gain, scale, T)
        self.ids = [int(i) for i in g[p + "ids"]]
        self.rows = [int(r) for r in g[p + "rows"]]
        self.ref = {r: tt(g[p + "logits"][i]).double() for i, r in enumerate(self.rows)}
        self.scale = float(g[p + "scale"])
        self.hf16 = g[p + "hf16"].astype(np.float64)
        self.margin = g[p + "margin"].astype(np.float64)
        self.worst16 = float(self.hf16.max())

    def bound(self, row):
        """1.5 x that row's HF-fp16 error, the case's worst HF-fp16 row being the floor (rows where fp16 happened to be lucky)"""
        return MARGIN * max(float(self.hf16[row]), self.worst16)

    def full(self, k):
        """prefix followed by the embeddings of the first k fixture ids"""
        if k == 0:
            return self.emb
        return torch.cat([self.emb, self.w["embed_tokens.weight"][torch.tensor(self.ids[:k])]], 0)

    def check_row(self, key, row, logits):
        """one row of GPU logits against the fp64 row: finite, inside the yardstick, and the same greedy id wherever the fp64 margin
        exceeds twice the bound (the margin rule of this suite)"""
        logits = logits.double().cpu()
        assert torch.isfinite(logits).all(), (self.name, row)
        b = self.bound(row)
        observe(key, (logits - self.ref[row]).abs().max().item() / self.scale, b)
        if self.margin[row] > 2 * b * self.scale:
            assert int(logits.argmax()) == int(self.ref[row].argmax()), (self.name, row)


def cases_of(combo):
    seed, gain, scale = combo
    return [Case(name, seed, gain, scale, T) for name, T in COMBOS[combo]]


def make_engine(w, max_batch, use_graph=False):
    from aurora_amd.engine import AuroraCapEngine
    e = AuroraCapEngine({"vit": None, "llm": CKPT_LLM_CFG}, {"llm": w}, max_frames=1, max_batch=max_batch, max_ctx=512,
                        max_new_tokens=NEW, use_graph=use_graph)
    if max_batch > 32:
        e.set_option("skinny_row_split_min_k", 128)      # tiny dims: both residual projections through the split-K + reduce path
    return e


def forced_decode_rows(eng, c):
    """GPU logits at rows T - 1 .. T + 14, teacher-forced on the FIXTURE's ids: prefill, then one decode step per token for as long as
    the engine's own pick is the fixture's id; where it is not (legitimate only at a near tie: check_row decides) the rows so far plus
    the fixture's tokens are prefilled as a longer prefix and the decode goes on from there."""
    out = []
    while len(out) < NEW:
        k = len(out)
        eng.begin_batch(1, NEW - k, None)
        eng.prefill(0, padded(c.full(k)), c.T + k)
        out.append(eng.logits()[0].cpu())
        while len(out) < NEW:
            picked = eng.outputs()[0]
            assert picked[-1] == int(torch.argmax(out[-1]))              # greedy = first argmax of the GPU's own logits
            if picked[-1] != c.ids[len(out) - 1]:
                break
            eng.decode(1)
            out.append(eng.logits()[0].cpu())
    return out


def check_decode_rows(eng, c, key):
    rows = forced_decode_rows(eng, c)
    for j, lg in enumerate(rows):
        c.check_row(key, c.T - 1 + j, lg)
    return rows


def free_run(eng, embs, lens):
    """ragged batch, 16 greedy tokens, the logits of every step: (ids, [NEW, B, V])"""
    eng.begin_batch(len(embs), NEW, None)
    for b, (e, L) in enumerate(zip(embs, lens)):
        eng.prefill(b, padded(e), L)
    logits = [eng.logits().clone()]
    for _ in range(NEW - 1):
        eng.decode(1)
        logits.append(eng.logits().clone())
    return eng.outputs(), torch.stack(logits)


# ----------------------------------------------------------------------------------------------- a / b: the Llama path
@pytest.mark.parametrize("combo", list(COMBOS), ids=COMBO_IDS)
def test_llama_rows_within_the_fp16_yardstick_per_wave_structure(combo):
    """Engine of 2 slots (decode projections: x per wave).  Every stored prefix row (a prefill of exactly that length: causal, so its
    last row is that row), every decode position; on the 300-token cases the decode attention with one page per split (five splits
    with content), two (three, the last partial) and a single split; the 256x256 prefill GEMMs bitwise the 128x128 ones; the cases as
    ragged slots of one batch bitwise each alone; hipGraph bitwise eager.  The gain-1 cases at scales 2^-10, 2^-6, 1 and 2^6 are the
    test of the sum(x^2) fixed point across its range: the final norm of every first token and every norm of a decode step read it
    (row 0 at 2^6 is the massive row itself: sum(x^2) 4e8, 1e17 in fixed point)."""
    cs = cases_of(combo)
    eng = make_engine(cs[0].w, 2)
    try:
        # ragged slots of one batch == each alone (== the hipGraph replay below), bit for bit; free running: nothing to teacher-force.
        # First, on the engine's own options: the option sweeps further down stay set
        pair = cs[-2:]
        embs, lens = [c.emb for c in pair], [c.T for c in pair]
        ids, lg = free_run(eng, embs, lens)
        for b in range(len(pair)):
            ids1, lg1 = free_run(eng, embs[b: b + 1], lens[b: b + 1])
            assert ids1[0] == ids[b] and torch.equal(lg1[:, 0], lg[:, b]), pair[b].name
        for c in cs:
            for r in [r for r in c.rows if r < c.T - 1]:
                eng.begin_batch(1, 1, None)
                eng.prefill(0, padded(c.emb[: r + 1]), r + 1)
                c.check_row(f"ckpt/llama_prefix_rows_over_scale[{c.name}]", r, eng.logits()[0])
            check_decode_rows(eng, c, f"ckpt/llama_decode_rows_over_scale[b2][{c.name}]")
            if c.T == 300:
                for pps in (1, 2, 1 << 20):
                    eng.set_option("dec_attn_pps", pps)
                    check_decode_rows(eng, c, f"ckpt/llama_decode_rows_over_scale[b2,pps{min(pps, 99)}][{c.name}]")
                first = []
                for mode in (0, 2, 1):
                    eng.set_option("gemm_mode", mode)
                    eng.begin_batch(1, 1, None)
                    eng.prefill(0, padded(c.emb), c.T)
                    first.append(eng.logits().clone())
                assert torch.equal(first[0], first[1]) and torch.equal(first[0], first[2])
    finally:
        eng.close()
    eng = make_engine(cs[0].w, 2, use_graph=True)
    try:
        ids_g, lg_g = free_run(eng, embs, lens)
        assert ids_g == ids and torch.equal(lg_g, lg), "hipGraph replay must reproduce the eager decode bit for bit"
    finally:
        eng.close()


@pytest.mark.parametrize("max_batch", [40, 128])
@pytest.mark.parametrize("combo", list(COMBOS), ids=COMBO_IDS)
def test_llama_rows_within_the_fp16_yardstick_lds_structure(combo, max_batch):
    """Engines of 40 and 128 slots (x through LDS; 128 also sums gate/up in one k pass and splits K of both residual projections):
    the first four prefix rows (row 0 at scale 2^6: sum(x^2) = 4e8 through this structure's `ssq_to_rstd`) and the decode rows inside the
    yardstick with `decode_fused_reduce` 0 and 1 (bitwise equal), the half-grid forms and the
    workgroup-local join of the attention splits on the 128-slot engine (bitwise equal), ragged batch == alone, hipGraph == eager."""
    cs = cases_of(combo)
    tag = f"b{max_batch}"
    eng = make_engine(cs[0].w, max_batch)
    try:
        embs, lens = [c.emb for c in cs], [c.T for c in cs]         # on the engine's own options, before the sweeps below
        ids, lg = free_run(eng, embs, lens)
        for b in range(len(cs)):
            ids1, lg1 = free_run(eng, embs[b: b + 1], lens[b: b + 1])
            assert ids1[0] == ids[b] and torch.equal(lg1[:, 0], lg[:, b]), cs[b].name
        for c in cs:
            for r in (0, 1, 2, 3):           # first tokens of 1 .. 4-row prefixes: this structure's lm_head reads sum(x^2) of the massive row
                eng.begin_batch(1, 1, None)
                eng.prefill(0, padded(c.emb[: r + 1]), r + 1)
                c.check_row(f"ckpt/llama_prefix_rows_over_scale[{tag}][{c.name}]", r, eng.logits()[0])
            rows = {}
            for fused in (0, 1):
                eng.set_option("decode_fused_reduce", fused)
                rows[fused] = check_decode_rows(eng, c, f"ckpt/llama_decode_rows_over_scale[{tag}][{c.name}]")
            eng.set_option("decode_fused_reduce", 0)
            assert all(torch.equal(a, b) for a, b in zip(rows[0], rows[1])), c.name
            if max_batch == 128:
                eng.set_option("decode_half_grid", 1)
                half = check_decode_rows(eng, c, f"ckpt/llama_decode_rows_over_scale[{tag}][{c.name}]")
                eng.set_option("decode_half_grid", 0)
                assert all(torch.equal(a, b) for a, b in zip(rows[0], half)), c.name
                if c.T == 300:           # 8 pages of capacity in 4 splits of 2: [2, 2, 1 (partial), 0] pages of this context
                    eng.set_option("dec_attn_pps", 2)
                    loc = {}
                    for local in (1, 0):
                        eng.set_option("dec_attn_local", local)
                        loc[local] = check_decode_rows(eng, c, f"ckpt/llama_decode_rows_over_scale[{tag},pps2][{c.name}]")
                    eng.set_option("dec_attn_local", 1)
                    assert all(torch.equal(a, b) for a, b in zip(loc[0], loc[1])), c.name
    finally:
        eng.close()
    eng = make_engine(cs[0].w, max_batch, use_graph=True)
    try:
        ids_g, lg_g = free_run(eng, embs, lens)
        assert ids_g == ids and torch.equal(lg_g, lg), "hipGraph replay must reproduce the eager decode bit for bit"
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------- c: the ViT layer
@pytest.mark.parametrize("name", list(CKPT_VIT_CASES))
def test_vit_layer_within_the_fp16_reference(name):
    """One encoder layer under checkpoint-like LayerNorm weights / biases and a residual stream with outlier channels: rel-L2 against
    the fp64 oracle (told the GPU's merge) at most 1.5x what the reference's own layer in torch.float16 shows against fp64 on the same
    input; indices bit-exact against the C restatement on the GPU's metric bytes; LayerNorm 2 out of the merge launch bitwise the
    separate launch."""
    from aurora_amd.engine import AuroraCapEngine
    g = golden("g17_ckpt_stats.npz")
    cfg, frames, r, wseed, xseed = CKPT_VIT_CASES[name]
    w = ckpt_like_vit_weights(cfg, wseed)
    t = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    x = ckpt_like_vit_input(xseed, frames, t, cfg["hidden_size"])
    eng = AuroraCapEngine({"vit": cfg, "llm": None}, {"vit": w}, max_frames=frames, max_batch=1, max_ctx=128, max_new_tokens=8)
    try:
        outs = []
        for fused in (1, 0):
            eng.set_option("tome_fused_ln", fused)
            xo, so, metric, idx = eng.vit_layer(0, x, None, r)
            outs.append((xo.cpu(), so.cpu(), metric.cpu(), {k: idx[k].cpu() for k in ("node_idx", "unm_idx", "src_idx", "dst_idx")}))
        eng.set_option("tome_fused_ln", 1)
        xo, so, metric, idx = outs[0]
        assert torch.equal(xo, outs[1][0]) and torch.equal(so, outs[1][1]) and torch.equal(metric, outs[1][2])
        mc = tome_ref.match(metric.numpy(), r)
        for k in ("node_idx", "unm_idx", "src_idx", "dst_idx"):
            np.testing.assert_array_equal(idx[k].numpy(), mc[k], err_msg=k)
            assert torch.equal(idx[k], outs[1][3][k]), k
        assert torch.isfinite(xo.float()).all()
        lwd = {k: v.double() for k, v in w["layers"][0].items()}
        ref, size = O.vit_layer(x.double(), None, lwd, cfg["num_attention_heads"], r, cfg["hidden_act"], forced_match=to_match(dict(idx, r=r)))
        bound = MARGIN * float(g[f"vit.{name}.ref16_rel_l2"])
        observe(f"ckpt/vit_layer_rel_l2[{name}]", rel_l2(xo.float(), ref), bound)
        np.testing.assert_array_equal(so.numpy(), size[..., 0].float().numpy())
        if all(np.array_equal(idx[k].numpy(), g[f"vit.{name}.{k}"]) for k in ("unm_idx", "src_idx", "dst_idx")):
            observe(f"ckpt/vit_layer_rel_l2_vs_fixture_rows[{name}]", rel_l2(xo.float(), tt(g[f"vit.{name}.out"])), bound)
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------- d / e: kernels against fp64
@pytest.fixture(scope="module")
def keng():
    from aurora_amd.engine import AuroraCapEngine
    cfg = {"vit": dict(hidden_size=1280, num_attention_heads=16, num_hidden_layers=2, intermediate_size=256, patch_size=14,
                       image_size=378, hidden_act="quick_gelu"), "llm": None}
    e = AuroraCapEngine(cfg, {}, max_frames=2, max_batch=1, max_ctx=128, max_new_tokens=8)
    yield e
    e.close()


def norm_rows(rows, d, g):
    """[rows, d] fp16: the rows norm kernels go wrong on, cycled"""
    x = torch.empty(rows, d)
    kinds = []
    for i in range(rows):
        k = ("offset", "spike", "subnormal", "ones", "zero")[i % 5]
        kinds.append(k)
        n = torch.randn(d, generator=g)
        if k == "offset":                      # mean >> std: the cancellation in x - mean
            x[i] = 50.0 + 0.1 * n
        elif k == "spike":                     # one element at 3e4 among 0.01 N: sum(x^2) = 9e8
            x[i] = 0.01 * n
            x[i, int(torch.randint(0, d, (1,), generator=g))] = 3e4
        elif k == "subnormal":                 # every element below fp16's smallest normal (6.1e-5)
            x[i] = (2e-5 * n).clamp(-6e-5, 6e-5)
        elif k == "ones":
            x[i] = 1.0
        else:
            x[i] = 0.0
    return x.half(), kinds


@pytest.mark.parametrize("rows,d", [(5, 64), (33, 4096), (7, 320)])
def test_norm_kernels_against_fp64_with_derived_bounds(keng, rows, d):
    """`norm_kernel` (norm.hip) is two-pass in fp32 on the row held in registers: each lane chains d / 64 terms, a 6-step wave tree joins
    the lanes, then y = fp16((x - mean) rstd w + b) (LayerNorm: one fma, one rounding) or fp16(w fp16(x rstd)) (RMSNorm: HF rounds the
    normalised value first: two roundings).  With x_hat and rstd from an fp64 evaluation the error of one element is therefore at most
        r 2^-11 (|x_hat w| + |b|)                         the fp16 roundings (r = 1 LayerNorm, r = 2 RMSNorm), half an ulp each
      + (d / 64 + 8) 2^-24 max|x| rstd |w|                 one fp32 rounding (2^-24 relative) per term of the longest chain (d / 64 lane
                                                           terms + 6 tree steps) in mean / variance, relative to the largest element the
                                                           chain carries, plus the rounding of x - mean and of rstd itself (+ 2)
      + 2^-24                                              where the output is an fp16 subnormal (absolute spacing 2^-24; RMSNorm: also
                                                           where the normalised value it rounds first is one, times |w|).
    Rows: mean >> std, one 3e4 spike, all-subnormal, all ones (sums exactly in fp32 in any order: LayerNorm must return EXACTLY
    fp16(bias)), all zero (RMSNorm: zero, not NaN).  A case that needs more is a finding, not a tolerance."""
    g = torch.Generator().manual_seed(rows * 31 + d)
    x, kinds = norm_rows(rows, d, g)
    w = (0.4 * torch.exp(0.7 * torch.randn(d, generator=g))).float()
    w[int(torch.randint(0, d, (1,), generator=g))] *= 0.02
    w[int(torch.randint(0, d, (1,), generator=g))] *= 8.0
    b = (0.5 * torch.randn(d, generator=g)).float()
    eps = float(np.float32(1e-5))
    xd, wd, bd = x.double(), w.double(), b.double()
    amax = xd.abs().amax(1, keepdim=True)
    chain = (d / 64 + 8) * 2.0 ** -24
    # LayerNorm
    mean = xd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (xd - mean) * rstd
    ref = xh * wd + bd
    bound = 2.0 ** -11 * ((xh * wd).abs() + bd.abs()) + chain * amax * rstd * wd.abs()
    bound = bound + (ref.abs() < 2.0 ** -14) * 2.0 ** -24
    out = keng.layernorm(x, w, b, 1e-5).cpu()
    assert torch.isfinite(out.float()).all()
    err = (out.double() - ref).abs()
    print("layernorm worst error / bound per row kind:", {k: float((err / bound)[i].max()) for i, k in enumerate(kinds[:5])})
    excess = (err - bound).amax(1)
    assert (excess <= 0).all(), [(kinds[i], float(excess[i])) for i in range(rows) if excess[i] > 0]
    for i, k in enumerate(kinds):
        if k in ("ones", "zero"):
            assert torch.equal(out[i], b.half()), k
    # RMSNorm
    rstd = 1.0 / torch.sqrt((xd ** 2).mean(1, keepdim=True) + eps)
    xh = xd * rstd
    ref = xh * wd
    bound = 2 * 2.0 ** -11 * ref.abs() + chain * amax * rstd * wd.abs()
    bound = bound + (ref.abs() < 2.0 ** -14) * 2.0 ** -24 + (xh.abs() < 2.0 ** -14) * 2.0 ** -24 * wd.abs()
    out = keng.rmsnorm(x, w, 1e-5).cpu()
    assert torch.isfinite(out.float()).all()
    err = (out.double() - ref).abs()
    print("rmsnorm worst error / bound per row kind:", {k: float((err / bound.clamp_min(1e-300))[i].max()) for i, k in enumerate(kinds[:5])})
    excess = (err - bound).amax(1)
    assert (excess <= 0).all(), [(kinds[i], float(excess[i])) for i in range(rows) if excess[i] > 0]
    for i, k in enumerate(kinds):
        if k == "zero":
            assert not out[i].any()


@pytest.mark.parametrize("m,n,k", [(77, 256, 1280), (2142, 512, 4096)])
def test_linear_with_outliers_against_fp64(keng, m, n, k):
    g = torch.Generator().manual_seed(m * 7 + n + 17)
    a, w = outlier_operands(m, n, k, g)
    ref = a.double() @ w.double().T
    bound = gemm_bound(a, w, ref, True)
    outs = {}
    try:
        for mode in (0, 2):                                    # the 128x128 kernel, the 256x256 kernel forced
            keng.set_option("gemm_mode", mode)
            outs[mode] = keng.linear(a, w, None).cpu()
            assert torch.isfinite(outs[mode].float()).all()
            excess = ((outs[mode].double() - ref).abs() - bound).max().item()
            assert excess <= 0, (mode, excess)
    finally:
        keng.set_option("gemm_mode", 1)
    assert torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("b,n,k", [(8, 384, 4096), (16, 128, 1024), (8, 256, 11008), (24, 128, 4096), (32, 384, 11008), (33, 256, 1024),
                                   (48, 128, 4096), (64, 384, 11008)])
def test_skinny_linear_with_outliers_against_fp64(keng, b, n, k):
    g = torch.Generator().manual_seed(b * 13 + n + 17)
    a, w = outlier_operands(b, n, k, g)
    ref = a.double() @ w.double().T
    out = keng.linear_skinny(a, w).cpu()
    assert torch.isfinite(out).all()
    excess = ((out.double() - ref).abs() - gemm_bound(a, w, ref, False)).max().item()
    assert excess <= 0, excess


@pytest.mark.parametrize("b,k,n", [(33, 4096, 1024), (48, 1024, 4096), (64, 11008, 256), (128, 11008, 128)])
def test_skinny_linear_through_lds_with_outliers_against_fp64(b, k, n):
    from aurora_amd.engine import AuroraCapEngine
    eng = AuroraCapEngine({"vit": None, "llm": None}, {}, max_frames=1, max_batch=128)       # > 32 slots: x through LDS
    try:
        g = torch.Generator().manual_seed(b * 13 + n + 19)
        a, w = outlier_operands(b, n, k, g)
        ref = a.double() @ w.double().T
        out = eng.linear_skinny(a, w).cpu()
        assert torch.isfinite(out).all()
        excess = ((out.double() - ref).abs() - gemm_bound(a, w, ref, False)).max().item()
        assert excess <= 0, excess
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------- f: the greedy pick on exact ties
def tied_lm_head(w, pairing, V):
    """lm_head with rows duplicated so that EVERY step's maximum is an exact tie: id hi gets the row of id lo < hi"""
    head = w["lm_head.weight"].clone()
    pairs = {}
    for lo, hi in pairing(V):
        assert lo < hi < V
        head[hi] = head[lo]
        pairs[lo], pairs[hi] = hi, lo
    return dict(w, **{"lm_head.weight": head}), pairs


PAIRINGS = {
    # within one 16-byte group of four logits (one thread's load; the scalar scan of v323: threads three apart)
    "same_load": lambda V: [(4 * i + j, 4 * i + 3 - j) for i in range(V // 4) for j in range(2)],
    # neighbouring threads of one wave
    "next_thread": lambda V: [(8 * i + j, 8 * i + 4 + j) for i in range(V // 8) for j in range(4)],
    # far apart: other waves of the block (v323: lanes 161 apart; v9000: ids 4500 apart)
    "other_wave": lambda V: [(i, i + V // 2) for i in range(V // 2)],
    # the same thread's second pass over a vocabulary of more than 4 x 1024 ids
    "next_pass": lambda V: [(i, i + 4096) for i in range(V - 4096)],
}
TIE_CASES = [(n, p) for n in ("v323", "v9000", "hd64") for p in PAIRINGS if p != "next_pass" or n == "v9000"]


@pytest.mark.parametrize("name,pairing", TIE_CASES)
def test_greedy_pick_on_exact_ties_takes_the_lower_id(name, pairing):
    """`argmax_advance_kernel` must pick what torch.argmax picks on the same fp32 logits: the FIRST maximum.  lm_head rows are
    duplicated at ids lo < hi (same 16-byte load, neighbouring threads, another wave, the same thread's next pass; a vocabulary that is
    a multiple of 4, one that is not - the scalar scan - and one of several passes), so every step's maximum is an exact tie: the id
    is the lower one over a 16-token decode, eager and as a hipGraph.  With EOS equal to a picked (lower) id the generation stops
    there, length and `finished` as HF's; with EOS equal to its duplicate (never picked) it runs to the end."""
    from aurora_amd.engine import AuroraCapEngine
    cfg = LLM_CFGS.get(name) or LLM_CFGS_VOCAB[name]
    V = cfg["vocab_size"]
    w, pairs = tied_lm_head(rand_llm_weights(cfg, 5), PAIRINGS[pairing], V)
    emb = torch.randn(40, cfg["hidden_size"], generator=torch.Generator().manual_seed(4)).half().float()

    def engine(use_graph):
        return AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": w}, max_frames=1, max_batch=1, max_ctx=256, max_new_tokens=NEW,
                               use_graph=use_graph)
    eng = engine(False)
    try:
        ids, lg = free_run(eng, [emb], [40])
        ids, lg = ids[0], lg[:, 0].cpu()
        assert len(ids) == NEW
        ties = 0
        for j in range(NEW):
            want = int(torch.argmax(lg[j]))                      # CPU: first maximum
            assert ids[j] == want, (j, ids[j], want)
            if want in pairs:
                assert lg[j, want] == lg[j, pairs[want]], "duplicated lm_head rows must give bitwise equal logits"
                assert want < pairs[want], (j, want, pairs[want])
                ties += 1
        assert ties >= NEW // 2, ties                             # (next_pass pairs 4904 of 9000 ids, an odd vocabulary leaves one out)
        # EOS at a picked id: stop there (the EOS itself is kept, HF semantics); at its never-picked duplicate: run to the end
        stop_at = next(j for j in range(3, NEW) if ids[j] in pairs)
        eos = ids[stop_at]
        first = ids.index(eos)
        stopped = eng.generate([padded(emb)], [40], NEW, eos_id=eos, check_every=4)[0]
        assert stopped == ids[: first + 1]
        lens, fin = eng.slot_state()
        assert int(lens[0]) == first + 1 and int(fin[0]) == 1 and eng.unfinished() == 0
        assert eng.generate([padded(emb)], [40], NEW, eos_id=pairs[eos], check_every=4)[0] == ids
    finally:
        eng.close()
    eng = engine(True)
    try:
        assert eng.generate([padded(emb)], [40], NEW, eos_id=None)[0] == ids
        assert eng.generate([padded(emb)], [40], NEW, eos_id=eos, check_every=4)[0] == ids[: first + 1]
    finally:
        eng.close()

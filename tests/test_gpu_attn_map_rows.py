"""The attention-map kernels alone - attn_map_score_kernel<KBLK> + attn_map_join_kernel (csrc/attn_map.hip) - against the fp64 definition,
elementwise, under the bound derived from their stated arithmetic (tests/attn_map_ref.py derived_bound; nothing here is an observed
tolerance).  They are reached through aur_attn_map_rows on the engines of tests/test_gpu_attention.py: the layer's own QKV launch with
the identity as weight writes exactly the caller's q into the query buffer and its k at pos_b into the pages, which the prefill entry
filled before - valid keys in front of pos_b, poison from there to the end of the context, whole later pages included.
tests/test_attn_map_reference.py shows on the CPU that a window or mask off by one, a missing newest key, a stale page count, one
page's normaliser, an empty page joined as m = 0, summed heads or layers and a missing 1 / sqrt(hd) leave this bound by more than 10x.

Worst error / bound seen on an MI355X: 0.020 (hd 32), 0.015 (hd 64), 0.014 (hd 128) without RoPE, 0.048 / 0.040 / 0.043 with it, 0.014 on
the engine of 18 pages.  Each test prints its own."""
import pytest
import torch

from tests.attn_map_ref import definition_fp64, derived_bound, worst_ratio
from tests.attn_ref import DEC_CASES, DEC_POS, rope_apply, rope_delta
from tests.test_gpu_attention import _ENGINES, CTX, CTX_BIG, SLOTS, as_rows, default_pps, engine, stack_cases
from tests.test_gpu_llm import LLM_CFGS

pytestmark = pytest.mark.gpu

WINDOWS = (64, 128, 384)


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e[0].close()
    _ENGINES.clear()


def fill(name, case, ctx, rope_on, pos):
    """pages of the 16 sequences: valid K at [0, pos_b), poison behind; -> (the step's rows x, q, k) with q, k [SLOTS, heads, ctx, hd]"""
    eng, layout, heads, hd, w, _ = engine(name)
    q, k, v = stack_cases(case, hd, [p + 1 for p in pos], ctx, heads, 177 + ctx, rope_safe=rope_on)
    kf, vf = k.clone(), v.clone()
    for b, p in enumerate(pos):             # the cache before the step: position pos_b is still poison
        kf[b, :, p], vf[b, :, p] = k[b, :, p + 1], v[b, :, p + 1]
    eng.attn_rows(as_rows(q, kf, vf), w, layout=layout, nseq=SLOTS, rows=ctx, causal=True, t=ctx, rope=rope_on)
    idx = torch.tensor(pos)
    step = lambda t: t[torch.arange(SLOTS), :, idx].reshape(SLOTS, heads * hd)          # row pos_b of every (sequence, head)
    return torch.cat([step(q), step(k), step(v)], 1), q, k


def references(name, q, k, pos, rope_on):
    """per slot: (q_b [1, H, hd], k_b [1, H, ctx, hd], delta) as the definition takes them - roped in fp64 when RoPE is on"""
    _, _, heads, hd, _, rope = engine(name)
    ctx = k.shape[-2]
    out = []
    for b, p in enumerate(pos):
        qb, kb, delta = q[b], k[b], 0.0
        if rope_on:
            ar = torch.arange(ctx)
            qb, kb = rope_apply(qb, ar, **rope), rope_apply(kb, ar, **rope)
            delta = rope_delta(qb[:, p:p + 1], kb, hd ** -0.5, (ar <= p)[None, :])
        out.append((qb[None, :, p], kb[None], delta))
    return out


def check_case(name, case, ctx, rope_on):
    eng, layout, heads, hd, w, _ = engine(name)
    pos = list(DEC_POS)
    x, q, k = fill(name, case, ctx, rope_on, pos)
    refs = references(name, q, k, pos, rope_on)
    worst = 0.0
    for W in WINDOWS:
        out = eng.attn_map_rows(x, w, pos, W, rope=rope_on)
        assert torch.equal(out, eng.attn_map_rows(x, w, pos, W, rope=rope_on)), ("not repeatable", W)
        out = out.cpu()
        assert torch.isfinite(out).all(), W
        for b, p in enumerate(pos):
            npos = p + 1
            qb, kb, delta = refs[b]
            assert not out[b, min(W, npos):].any(), (case, W, p, "columns at or beyond npos must be exactly 0.0")
            if W >= npos:
                assert abs(float(out[b].double().sum()) - 1.0) <= npos * 2.0 ** -22, (case, W, p, float(out[b].double().sum()))
            ref = definition_fp64(qb, kb, npos, W)
            r = worst_ratio(out[b], ref.a, derived_bound(ref, W, hd, (npos + 63) // 64, delta))
            assert r <= 1.0, (case, "window", W, "pos", p, r)
            worst = max(worst, r)
    return worst


@pytest.mark.parametrize("case", DEC_CASES + ("rand+rope",))
@pytest.mark.parametrize("name", list(LLM_CFGS))
def test_attn_map_rows(name, case):
    """one ragged launch, pos each side of the 16-token fragment row and the 64-token page up to five pages; windows shorter and longer
    than the contexts; poison keys and whole poison pages behind npos"""
    worst = check_case(name, case.split("+")[0], CTX, "+rope" in case)
    print(f"attention map {name} {case}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("case", DEC_CASES)
def test_attn_map_rows_with_eighteen_pages(case):
    """an engine of 1152 positions: 18 pages per sequence, most of them behind the context of most sequences"""
    worst = check_case("hd64@big", case, CTX_BIG, False)
    print(f"attention map hd64, 18 pages, {case}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", list(LLM_CFGS))
def test_attn_map_rows_do_not_depend_on_geometry_or_batch(name):
    """bitwise the same under every split geometry of the decode attention and at batch 1, 3 and 16 (the longest contexts first)"""
    eng, layout, heads, hd, w, _ = engine(name)
    pos = list(reversed(DEC_POS))
    x, _, _ = fill(name, "rand", CTX, False, pos)
    dflt = default_pps(heads, CTX // 64)
    base = eng.attn_map_rows(x, w, pos, 384)
    assert float(base[0, :320].min()) > 0.0
    try:
        for pps in (1, 2, 6):
            for local in (0, 1):
                eng.set_option("dec_attn_pps", pps)
                eng.set_option("dec_attn_local", local)
                assert torch.equal(base, eng.attn_map_rows(x, w, pos, 384)), (pps, local)
        for n in (1, 3):
            assert torch.equal(base[:n], eng.attn_map_rows(x[:n], w, pos[:n], 384)), n
        assert torch.equal(base[:, :128], eng.attn_map_rows(x, w, pos, 128)), "a shorter window is a prefix of a longer one"
    finally:
        eng.set_option("dec_attn_pps", dflt)
        eng.set_option("dec_attn_local", 1)


def test_attn_map_rows_reject_bad_arguments():
    from aurora_amd._lib import AuroraHipError
    eng, layout, heads, hd, w, _ = engine("hd32")
    x = torch.zeros(2, 3 * heads * hd)
    for W in (0, 32, 96, CTX + 64):
        with pytest.raises(AuroraHipError, match="status -1"):
            eng.attn_map_rows(x, w, [0, 0], W)
    with pytest.raises(AuroraHipError, match="status -1"):
        eng.attn_map_rows(torch.zeros(SLOTS + 1, 3 * heads * hd), w, [0] * (SLOTS + 1), 64)
    assert eng.L.aur_attn_map_bytes(eng.ctx, 96) == -1 and eng.L.aur_attn_map_bytes(eng.ctx, 128) > 0
    out = eng.attn_map_rows(x, w, [0, 0], 64).cpu()                 # the ctx is still usable: one key, p = 1
    assert torch.equal(out[:, 0], torch.ones(2)) and not out[:, 1:].any()

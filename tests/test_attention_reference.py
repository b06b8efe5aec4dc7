"""CPU checks of tests/attn_ref.py, which make the strength of tests/test_gpu_attention.py checkable without a GPU:
  * the emulator (the kernels' stated arithmetic: fp32 scores, online softmax over 64-key blocks, p rounded to fp16, fp32 sums, fp16
    output, optional page splits joined in fp32) stays inside derived_bound for every case and shape the GPU test runs - and still
    does with the fp32 coefficient halved, so the bound holds without leaning on that coefficient;
  * every mutation of the emulator (an off-by-one mask, a missing newest key, an ignored page, a mishandled empty split, a missing
    rescale) leaves the bound by at least 100x in at least one case at EVERY shape it applies to - so a kernel with that error cannot
    pass the GPU test;
  * the `future` and `newest` constructions put >= 0.99 of the weight on the intended key.
Figures of the last run (printed by the tests): emulator worst error / bound 0.88 (flash form), 0.62 (decode form), unchanged to
two digits with the fp32 coefficient halved; weakest mutant margin 737x."""
import math

import pytest
import torch

from tests.attn_ref import (DEC_CASES, DEC_POS, FLASH_CASES, T_LIST, attention_fp64, build_case, derived_bound, emulate, flash_shapes,
                            rope_apply, rope_delta, rup, split_ranges, visible, worst_ratio)

FLASH_HDS = (16, 32, 64, 80, 128)
DEC_HDS = (32, 64, 128)
ROPE = dict(theta=1e4, factor=4.0)
# (pages of a sequence, pages per split): the splits of an engine of 384 positions - default (1), 2, 4, beyond the context (one split:
# the kernel normalises and stores itself) - and the 18 single-page splits of an engine of 1152 positions (the combine's generic loop)
DEC_SPLITS = ((6, 1), (6, 2), (6, 4), (6, 6), (18, 1))
MUTANT_MARGIN = 100.0


def _seed(*parts):
    h = 0
    for p in parts:
        h = (h * 1000003 + (hash(p) if not isinstance(p, str) else sum(ord(c) * (i + 1) for i, c in enumerate(p)))) % (2 ** 31)
    return h


def flash_case(name, hd, n_valid, rows, causal, rope=False):
    """(q, k, v as the kernel stores them, reference, Delta): queries are the valid rows"""
    q, k, v = build_case(name, hd, n_valid, rows, _seed(name, hd, n_valid, rows, causal), rope_safe=rope)
    scale, delta = hd ** -0.5, 0.0
    q64, k64 = q, k
    if rope:
        pos = torch.arange(rows)
        q64, k64 = rope_apply(q, pos, **ROPE), rope_apply(k, pos, **ROPE)
        delta = rope_delta(q64[:n_valid], k64, scale, visible(n_valid, rows, causal, n_valid))
        q, k = rope_apply(q, pos, dtype=torch.float32, **ROPE).half().float(), rope_apply(k, pos, dtype=torch.float32, **ROPE).half().float()
    ref = attention_fp64(q64[:n_valid], k64, v, scale, causal, n_valid)
    return (q[:n_valid], k, v), ref, delta


def dec_case(name, hd, pos, rope=False):
    """one decode step at `pos` cached tokens: the query is row pos, keys [0, pos] are visible, poison from pos + 1 to the page's end"""
    n_valid, rows = pos + 1, rup(pos + 2, 64)
    q, k, v = build_case(name, hd, n_valid, rows, _seed("dec", name, hd, pos), rope_safe=rope)
    scale, delta = hd ** -0.5, 0.0
    q64, k64 = q, k
    if rope:
        p = torch.arange(rows)
        q64, k64 = rope_apply(q, p, **ROPE), rope_apply(k, p, **ROPE)
        delta = rope_delta(q64[pos:pos + 1], k64, scale, visible(1, rows, False, n_valid))
        q, k = rope_apply(q, p, dtype=torch.float32, **ROPE).half().float(), rope_apply(k, p, dtype=torch.float32, **ROPE).half().float()
    ref = attention_fp64(q64[pos:pos + 1], k64, v, scale, False, n_valid)
    return (q[pos:pos + 1], k, v), ref, delta


@pytest.mark.parametrize("hd", FLASH_HDS)
def test_emulator_stays_inside_the_bound_flash_form(hd):
    worst, worst_half, at = 0.0, 0.0, None
    for n_valid, rows in flash_shapes():
        for causal in (False, True):
            for name in FLASH_CASES + (("rand+rope",) if hd >= 32 and causal else ()):
                if name == "future" and not causal:
                    continue
                (q, k, v), ref, delta = flash_case(name.split("+")[0], hd, n_valid, rows, causal, rope="+rope" in name)
                got = emulate(q, k, v, hd ** -0.5, causal, n_valid)
                r = worst_ratio(got, ref.o, derived_bound(ref, 1, delta))
                if r > worst:
                    worst, at = r, (name, n_valid, rows, causal)
                worst_half = max(worst_half, worst_ratio(got, ref.o, derived_bound(ref, 1, delta, c32_scale=0.5)))
    print(f"flash form hd {hd}: emulator worst error / bound {worst:.3f} at {at}; with the fp32 coefficient halved {worst_half:.3f}")
    assert worst <= 1.0 and worst_half <= 1.0


@pytest.mark.parametrize("hd", DEC_HDS)
def test_emulator_stays_inside_the_bound_decode_form(hd):
    worst, worst_half, at = 0.0, 0.0, None
    for pos in DEC_POS:
        for name in DEC_CASES + ("rand+rope",):
            (q, k, v), ref, delta = dec_case(name.split("+")[0], hd, pos, rope="+rope" in name)
            for pages, pps in DEC_SPLITS:
                ranges = split_ranges(pages, pps)
                got = emulate(q, k, v, hd ** -0.5, False, pos + 1, ranges=ranges)
                r = worst_ratio(got, ref.o, derived_bound(ref, len(ranges), delta))
                if r > worst:
                    worst, at = r, (name, pos, pages, pps)
                worst_half = max(worst_half, worst_ratio(got, ref.o, derived_bound(ref, len(ranges), delta, c32_scale=0.5)))
    print(f"decode form hd {hd}: emulator worst error / bound {worst:.3f} at {at}; with the fp32 coefficient halved {worst_half:.3f}")
    assert worst <= 1.0 and worst_half <= 1.0


def _flash_mutant(mut, hd, n_valid, rows, causal):
    """largest error / bound over the cases, with mutation `mut`"""
    best = 0.0
    for name in FLASH_CASES:
        if name == "future" and not causal:
            continue
        (q, k, v), ref, delta = flash_case(name, hd, n_valid, rows, causal)
        best = max(best, worst_ratio(emulate(q, k, v, hd ** -0.5, causal, n_valid, mut=(mut,)), ref.o, derived_bound(ref, 1, delta)))
    return best


@pytest.mark.parametrize("hd", FLASH_HDS)
def test_mask_and_rescale_mutants_leave_the_bound_flash_form(hd):
    """causal off by one: every shape with a second valid key.  tail off by one: every non-causal shape that has a row behind the valid
    ones (rows == n_valid has no key n_valid to leak; under a causal mask with n_valid by value key n_valid is never at or below a valid
    query, so that mutant is redundant by construction and is not asserted).  never rescale: every shape with a second key block."""
    weakest = math.inf
    for n_valid, rows in flash_shapes():
        if n_valid > 1:
            weakest = min(weakest, m := _flash_mutant("causal", hd, n_valid, rows, True))
            assert m >= MUTANT_MARGIN, ("causal", hd, n_valid, rows, m)
        if rows > n_valid:
            weakest = min(weakest, m := _flash_mutant("tail", hd, n_valid, rows, False))
            assert m >= MUTANT_MARGIN, ("tail", hd, n_valid, rows, m)
        if n_valid > 64:
            for causal in (False, True):
                weakest = min(weakest, m := _flash_mutant("never_rescale", hd, n_valid, rows, causal))
                assert m >= MUTANT_MARGIN, ("never_rescale", hd, n_valid, rows, causal, m)
    print(f"flash form hd {hd}: weakest mutant margin {weakest:.0f}x the bound")


@pytest.mark.parametrize("hd", DEC_HDS)
def test_mutants_leave_the_bound_decode_form(hd):
    """tail off by one (key pos + 1 is poison; it sits in a page the step reads unless pos + 1 starts a new page), the step's own key
    missing, the newest page ignored: every position.  An empty split joined as (m = 0, l = 0): every (position, split geometry) with a
    split behind the newest page.  Never rescale: every geometry whose first split holds a second page of visible keys."""
    weakest = math.inf
    for pos in DEC_POS:
        cases = [(name,) + dec_case(name, hd, pos) for name in DEC_CASES]

        def margin(mut, ranges):
            return max(worst_ratio(emulate(q, k, v, hd ** -0.5, False, pos + 1, ranges=ranges, mut=(mut,)), ref.o,
                                   derived_bound(ref, len(ranges), delta)) for _, (q, k, v), ref, delta in cases)
        for pages, pps in DEC_SPLITS:
            ranges = split_ranges(pages, pps)
            todo = ["newest", "last_page"]
            if (pos + 1) % 64:
                todo.append("tail")
            if any(k0 > pos for k0, _ in ranges):
                todo.append("empty_join")
            if pos >= 64 and pps > 1:
                todo.append("never_rescale")
            for mut in todo:
                weakest = min(weakest, m := margin(mut, ranges))
                assert m >= MUTANT_MARGIN, (mut, hd, pos, pages, pps, m)
    print(f"decode form hd {hd}: weakest mutant margin {weakest:.0f}x the bound")


@pytest.mark.parametrize("hd", FLASH_HDS)
def test_future_and_newest_put_the_weight_on_the_intended_key(hd):
    for n_valid in T_LIST:
        q, k, v = build_case("future", hd, n_valid, rup(n_valid, 32), 7)
        p = attention_fp64(q[:n_valid], k, v, hd ** -0.5, True, n_valid).p
        assert float(p.diagonal().min()) >= 0.99, (hd, n_valid, float(p.diagonal().min()))
    for pos in DEC_POS:
        q, k, v = build_case("newest", hd, pos + 1, rup(pos + 2, 64), 7)
        p = attention_fp64(q[pos:pos + 1], k, v, hd ** -0.5, False, pos + 1).p
        assert float(p[0, pos]) >= 0.99, (hd, pos, float(p[0, pos]))

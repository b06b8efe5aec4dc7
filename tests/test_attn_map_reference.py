"""CPU side of the attention-map tests: the fp32 emulator of csrc/attn_map.hip's stated arithmetic stays inside the bound of
tests/attn_map_ref.py at every shape of the GPU test, each of the errors that test must catch leaves it by more than 10x at every shape
where it can act, `attn_map.to_patches` against a brute-force loop, the numpy definition against the torch one, and the argument
checks of the Python surface."""
import functools
import math

import numpy as np
import pytest
import torch

from aurora_amd import attn_map as AM
from tests.attn_map_ref import MUTATIONS, definition_fp64, derived_bound, emulate, worst_ratio
from tests.attn_ref import DEC_CASES, DEC_POS, build_case, rope_apply, rope_delta

CTX, MAX_PAGES = 384, 6
WINDOWS = (64, 128, 384)
HEADS = {32: 4, 64: 4, 128: 2}


@functools.lru_cache(maxsize=None)
def case(name, hd, pos, layers=1):
    """q [L, H, hd] (the step's query: row pos), k [L, H, CTX, hd] (rows beyond pos poison)"""
    H = HEADS[hd]
    qs, ks = [], []
    for l in range(layers):
        qk = [build_case(name, hd, pos + 1, CTX, 9000 + pos * 64 + l * 16 + h) for h in range(H)]
        qs.append(torch.stack([t[0][pos] for t in qk]))
        ks.append(torch.stack([t[1] for t in qk]))
    return torch.stack(qs), torch.stack(ks)


@pytest.mark.parametrize("hd", sorted(HEADS))
def test_emulator_stays_inside_the_bound(hd):
    worst, worst_half = 0.0, 0.0
    for name in DEC_CASES:
        for pos in DEC_POS:
            q, k = case(name, hd, pos)
            npages = (pos + 1 + 63) // 64
            for W in WINDOWS:
                ref = definition_fp64(q, k, pos + 1, W)
                got = emulate(q, k, pos + 1, W, MAX_PAGES)
                assert not got[min(W, pos + 1):].any(), "columns at or beyond npos must be exactly zero"
                worst = max(worst, worst_ratio(got, ref.a, derived_bound(ref, W, hd, npages)))
                worst_half = max(worst_half, worst_ratio(got, ref.a, derived_bound(ref, W, hd, npages, c32_scale=0.5)))
    print(f"emulator hd {hd}: worst error / bound {worst:.4f} ({worst_half:.4f} with half the c32 term)")
    assert worst <= 1.0 and worst_half <= 1.0


def test_emulator_with_two_layers_and_rope_stays_inside_the_bound():
    hd = 64
    for pos in (63, 64, 300):
        q, k = case("rand", hd, pos, 2)
        q, k = q * 0.25, k * 0.25                                  # |q||k| scale small enough for rope_delta to stay small
        kr = rope_apply(k, torch.arange(CTX), 1e4, 1.0)
        qr = rope_apply(q[..., None, :], torch.tensor([pos]), 1e4, 1.0)[..., 0, :]
        ok = (torch.arange(CTX) <= pos)[None, :]
        delta = max(rope_delta(qr[l, h][None], kr[l, h], hd ** -0.5, ok) for l in range(2) for h in range(HEADS[hd]))
        ref = definition_fp64(qr, kr, pos + 1, 128)
        got = emulate(qr.half().float(), kr.half().float(), pos + 1, 128, MAX_PAGES)
        assert worst_ratio(got, ref.a, derived_bound(ref, 128, hd, (pos + 64) // 64, delta)) <= 1.0


def can_act(mut, pos):
    npos = pos + 1
    return {"tail": npos % 64 != 0,                 # the key behind the context lies in a page the kernel never opens
            "first_norm": npos > 64,                # a single page is its own normaliser
            "no_scale": npos > 1}.get(mut, True)    # one key: p = 1 whatever the scale


@pytest.mark.parametrize("mut", MUTATIONS)
@pytest.mark.parametrize("hd", sorted(HEADS))
def test_each_mutation_leaves_the_bound(hd, mut):
    """at every (hd, pos) where the error can act, at least one case and window sees it by more than 10x the bound"""
    layers = 2 if mut == "layers_sum" else 1
    skipped = []
    for pos in DEC_POS:
        if not can_act(mut, pos):
            skipped.append(pos)
            continue
        best = 0.0
        for name in DEC_CASES:
            q, k = case(name, hd, pos, layers)
            for W in WINDOWS:
                ref = definition_fp64(q, k, pos + 1, W)
                got = emulate(q, k, pos + 1, W, MAX_PAGES, mut=(mut,))
                best = max(best, worst_ratio(got, ref.a, derived_bound(ref, W, hd, (pos + 64) // 64)))
        assert best > 10.0, (mut, hd, pos, best)
    print(f"{mut} hd {hd}: cannot act at pos {skipped}")
    assert len(skipped) < len(DEC_POS)


def test_numpy_definition_matches_the_torch_one():
    q, k = case("rand", 32, 129, 2)
    ref = definition_fp64(q, k, 130, 128)
    row = AM.record_row(q.numpy(), k[..., :130, :].numpy(), 128)
    assert np.allclose(row, ref.a.numpy(), rtol=1e-12, atol=1e-300)
    short = AM.record_row(q.numpy()[:, :, :], k[..., :10, :].numpy(), 64)
    assert not short[10:].any() and abs(short.sum() - 1.0) < 1e-12


def test_to_patches_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    frames, gh, gw, n_kept, n = 3, 4, 5, 7, 6
    m = rng.integers(0, n_kept, size=(frames, gh, gw))
    m[0][m[0] == 3] = 2                                            # a token that stands for no patch
    va = rng.random((n, frames * n_kept))
    heat = AM.to_patches(va, m)
    assert heat.shape == (n, frames, gh, gw)
    for i in range(n):
        for f in range(frames):
            for y in range(gh):
                for x in range(gw):
                    t = m[f, y, x]
                    cnt = sum(1 for yy in range(gh) for xx in range(gw) if m[f, yy, xx] == t)
                    assert heat[i, f, y, x] == va[i, f * n_kept + t] / cnt
            used = sorted(set(m[f].reshape(-1).tolist()))
            assert math.isclose(heat[i, f].sum(), sum(va[i, f * n_kept + t] for t in used), rel_tol=1e-12)
    flat = AM.to_patches(va, m.reshape(frames, -1))
    assert np.array_equal(flat, heat.reshape(n, frames, -1))
    img = AM.render(heat, patch=3, gap=1)
    assert img.dtype == np.uint8 and img.shape == (n * (gh * 3 + 1) - 1, frames * (gw * 3 + 1) - 1, 3)
    y, x = np.unravel_index(heat[0, 0].argmax(), (gh, gw))
    hot = np.unravel_index(heat[0].reshape(-1).argmax(), heat[0].shape)
    assert (img[hot[1] * 3, hot[0] * (gw * 3 + 1) + hot[2] * 3] == 255).all()          # the hottest patch of a token's row is white
    with pytest.raises(ValueError):
        AM.to_patches(va, np.full((frames, gh, gw), n_kept))
    with pytest.raises(ValueError):
        AM.to_patches(va[:, :-1], m)


def test_visual_columns():
    a = np.arange(12, dtype=np.float32).reshape(2, 6)
    v = AM.visual(a, [1, 2, 4, 9])
    assert np.array_equal(v, np.array([[1, 2, 4, 0], [7, 8, 10, 0]], np.float32))
    with pytest.raises(ValueError):
        AM.visual(a, [-1])


def test_argument_checks():
    assert AM.check_attn_map(None) is None
    assert AM.check_attn_map({}) == (None, None)
    assert AM.check_attn_map(dict(keys=128, layers=[3, 1])) == (128, (1, 3))
    assert AM.check_attn_map(dict(keys=None, layers=[-1]), 4) == (None, (3,))
    assert AM.layer_mask(None) == 0 and AM.layer_mask((1, 3)) == 0b1010
    assert AM.window_for(1) == 64 and AM.window_for(64) == 64 and AM.window_for(65) == 128
    for bad in (True, 3, dict(keys=100), dict(keys=0), dict(keys=True), dict(keys=64.0), dict(layers=[]), dict(layers=[1, 1]), dict(layers=2),
                dict(layers=[1.5]), dict(layers="01"), dict(keys=64, other=1), dict(layers=[64])):
        with pytest.raises(ValueError):
            AM.check_attn_map(bad)
    with pytest.raises(ValueError):
        AM.check_attn_map(dict(layers=[4]), 4)
    with pytest.raises(ValueError):
        AM.check_attn_map(dict(layers=[-1]))

"""GPU: the merge map - which patches each visual token stands for - through the C ABI, against aurora_amd/merge_map.py (the numpy
definition) and the reference's own results (tests/golden/g20_merge_source.npz).  Integers and copies: every comparison is exact.

  1. aur_tome_map_rows alone: the seven fixture chains layer by layer, then edge shapes on indices made by the definition;
  2. aur_unmerge_rows: bitwise against torch.gather and against the reference's unmerge chain;
  3. aur_tome_step's own index outputs fed to aur_tome_map_rows;
  4. aur_vit_encode_map on random ViTs: the wiring into the layer loop;
  5. AuroraModel / inference.py on tests/golden/ckpt_tiny."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from aurora_amd import merge_map as MM
from tests.util import rand_vit_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g20_merge_source.npz"))
CASES = [str(c) for c in G["cases"]]
TINY = os.path.join(ROOT, "tests", "golden", "ckpt_tiny")

VIT_TINY = dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=4, intermediate_size=128, patch_size=14, image_size=56,
                hidden_act="quick_gelu", layer_norm_eps=1e-5)                      # the tiny random ViT of tests/test_gpu_vit.py: T0 = 17
VIT_MID = dict(hidden_size=320, num_attention_heads=4, num_hidden_layers=4, intermediate_size=640, patch_size=14, image_size=378,
               hidden_act="quick_gelu", layer_norm_eps=1e-5)                       # D = 320, T0 = 730
MAX_FRAMES = {"tiny": 4, "mid": 2}


def _engine(cfg, frames, seed):
    from aurora_amd.engine import AuroraCapEngine
    return AuroraCapEngine({"vit": cfg, "llm": None}, {"vit": rand_vit_weights(cfg, seed)}, max_frames=frames, max_batch=1, max_ctx=128,
                           max_new_tokens=8)


@pytest.fixture(scope="module")
def tiny():
    e = _engine(VIT_TINY, MAX_FRAMES["tiny"], 51)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mid():
    e = _engine(VIT_MID, MAX_FRAMES["mid"], 52)
    yield e
    e.close()


def dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def random_step(rng, frames, t, r):
    """valid index arrays of one step, as the select kernel would write them: unm ascending with the class row, src in any order"""
    ta, tb = (t + 1) // 2, t // 2
    unm, src, dst = np.zeros((frames, ta - r), np.int32), np.zeros((frames, r), np.int32), np.zeros((frames, r), np.int32)
    for f in range(frames):
        perm = 1 + rng.permutation(ta - 1)
        src[f] = perm[:r]
        unm[f] = np.sort(np.concatenate([[0], perm[r:]]))
        dst[f] = rng.integers(0, max(tb, 1), size=r)
    return unm, src, dst


# ---------------------------------------------------------------------------------------------- 1. aur_tome_map_rows alone
@pytest.mark.parametrize("name", CASES)
def test_map_rows_chains_the_fixture_to_the_reference_group(tiny, name):
    frames, t0, r, layers, _ = (int(v) for v in G[f"{name}_meta"])
    rows = dev(np.tile(np.arange(t0, dtype=np.int32), (frames, 1)))
    t = t0
    for l in range(layers):
        unm, src, dst = (G[f"{name}_L{l}_{k}"] for k in ("unm", "src", "dst"))
        rl = src.shape[1]
        assert rl == MM.clamp_r(t, r)
        tiny.tome_map_rows(rows, t, rl, dev(unm), dev(src), dev(dst))
        t -= rl
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rows.cpu().numpy(), G[f"{name}_group"])


def test_map_rows_edge_shapes_against_the_definition(tiny):
    rng = np.random.default_rng(77)
    done = 0
    for t in (2, 3, 4, 5, 731, 8192):
        for r in sorted({0, 1, (t - 1) // 2}):
            if r > (t - 1) // 2:
                continue
            for n in (1, 729, 8191):
                for frames in (1, 3, MAX_FRAMES["tiny"]):
                    unm, src, dst = random_step(rng, frames, t, r)
                    rows = rng.integers(0, t, size=(frames, n)).astype(np.int32)
                    want = np.stack([MM.step_rows(t, unm[f], src[f], dst[f])[rows[f]] for f in range(frames)]) if r else rows
                    got = tiny.tome_map_rows(dev(rows), t, r, dev(unm), dev(src), dev(dst))
                    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"t {t} r {r} n {n} frames {frames}")
                    done += 1
    assert done == (1 + 2 + 2 + 3 + 3 + 3) * 9


def test_map_rows_clamps_entries_and_stays_inside_its_buffer(tiny):
    rng = np.random.default_rng(78)
    frames, n, t, r = 3, 729, 731, 100
    unm, src, dst = random_step(rng, frames, t, r)
    rows = rng.integers(0, t, size=(frames, n)).astype(np.int32)
    rows[:, ::7] = np.array([-5, t, t + 100, 2 ** 31 - 1, -2 ** 31], np.int64)[rng.integers(0, 5, size=rows[:, ::7].shape)].astype(np.int32)
    buf = torch.full((frames * n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    view = buf[1:-1].view(frames, n)
    view.copy_(dev(rows))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4
    tiny.tome_map_rows(view, t, r, dev(unm), dev(src), dev(dst))
    got = buf.cpu().numpy()
    want = np.stack([MM.step_rows(t, unm[f], src[f], dst[f])[np.clip(rows[f], 0, t - 1)] for f in range(frames)])
    np.testing.assert_array_equal(got[1:-1].reshape(frames, n), want)
    assert got[0] == 0x5A5A5A5A and got[-1] == 0x5A5A5A5A            # the words just before and just behind the buffer


def test_map_rows_refuses_bad_arguments_and_the_ctx_survives(tiny):
    rows = dev(np.arange(10, dtype=np.int32).reshape(1, 10))
    idx = dev(np.zeros((1, 4096), np.int32))
    raw = lambda t, r, n=10, frames=1: tiny.L.aur_tome_map_rows(tiny.ctx, rows.data_ptr(), frames, n, t, r, idx.data_ptr(), idx.data_ptr(),
                                                                 idx.data_ptr(), tiny._stream())
    assert raw(8193, 1) == -1 and raw(9, 5) == -1 and raw(9, -1) == -1 and raw(0, 0) == -1 and raw(9, 1, n=0) == -1 and raw(9, 1, frames=0) == -1
    assert raw(2, 1) == -1                                            # (t - 1) / 2 = 0
    assert tiny.L.aur_tome_map_rows(tiny.ctx, rows.data_ptr(), 1, 10, 9, 1, None, idx.data_ptr(), idx.data_ptr(), tiny._stream()) == -1
    assert raw(9, 0) == 0                                             # r = 0: a no-op
    torch.cuda.synchronize()
    assert rows.cpu().numpy().tolist() == [list(range(10))]
    with pytest.raises(ValueError):
        tiny.tome_map_rows(rows, 9, 5, idx, idx, idx)
    with pytest.raises(ValueError):
        tiny.tome_map_rows(rows, 9, 2, idx[:, :2], idx[:, :2], idx[:, :2])          # unm must hold ceil(t / 2) - r = 3
    unm, src, dst = random_step(np.random.default_rng(1), 1, 10, 4)                  # and the ctx still works
    got = tiny.tome_map_rows(rows, 10, 4, dev(unm), dev(src), dev(dst)).cpu().numpy()
    np.testing.assert_array_equal(got[0], MM.step_rows(10, unm[0], src[0], dst[0]))


# ---------------------------------------------------------------------------------------------- 2. aur_unmerge_rows
@pytest.mark.parametrize("d", [8, 64, 1280])
def test_unmerge_bitwise_against_gather_with_sentinels(tiny, d):
    gen = torch.Generator().manual_seed(100 + d)
    frames, n_kept, n = 3, 37, 101
    tokens = torch.randn(frames, n_kept, d, generator=gen).half().cuda()
    mp = torch.randint(0, n_kept, (frames, n), generator=gen).cuda()
    want = torch.gather(tokens, 1, mp[..., None].expand(frames, n, d))
    got = tiny.unmerge(tokens, mp)
    assert got.shape == (frames, n, d) and got.dtype == torch.float16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(tiny.unmerge(tokens, mp.view(frames, 1, n)).view(torch.int16), want.view(frames, 1, n, d).view(torch.int16))
    # the raw call into a buffer with sentinel halves behind it; entries outside [0, n_kept) are clamped
    tail = 64
    buf = torch.full((frames * n * d + tail,), 0x5A5A, dtype=torch.int16, device="cuda")
    wild = mp.to(torch.int32).contiguous()
    wild[:, 0], wild[:, 1] = -3, n_kept + 5
    rc = tiny.L.aur_unmerge_rows(tiny.ctx, tokens.data_ptr(), wild.data_ptr(), frames, n, n_kept, d, buf.data_ptr(), tiny._stream())
    assert rc == 0
    torch.cuda.synchronize()
    want2 = torch.gather(tokens, 1, wild.long().clamp(0, n_kept - 1)[..., None].expand(frames, n, d))
    assert torch.equal(buf[:-tail].view(frames, n, d), want2.view(torch.int16))
    assert bool((buf[-tail:] == 0x5A5A).all())


@pytest.mark.parametrize("name", CASES)
def test_unmerge_bitwise_against_the_reference_chain(tiny, name):
    x, group, want = G[f"{name}_x"], G[f"{name}_group"], G[f"{name}_unmerged"]
    got = tiny.unmerge(torch.from_numpy(x), torch.from_numpy(group))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))


def test_unmerge_refuses_d_20_and_the_ctx_survives(tiny):
    tokens = torch.randn(1, 5, 20).half().cuda()
    mp = torch.zeros(1, 7, dtype=torch.int32, device="cuda")
    out = torch.zeros(1, 7, 20, dtype=torch.float16, device="cuda")
    assert tiny.L.aur_unmerge_rows(tiny.ctx, tokens.data_ptr(), mp.data_ptr(), 1, 7, 5, 20, out.data_ptr(), tiny._stream()) == -1
    assert b"multiple of 8" in tiny.L.aur_last_error(tiny.ctx)
    assert tiny.L.aur_unmerge_rows(tiny.ctx, tokens.data_ptr(), mp.data_ptr(), 1, 7, 0, 16, out.data_ptr(), tiny._stream()) == -1
    torch.cuda.synchronize()
    assert not out.any()
    t16 = torch.randn(1, 5, 16).half().cuda()
    assert torch.equal(tiny.unmerge(t16, mp), t16[:, :1].expand(1, 7, 16))


# ---------------------------------------------------------------------------------------------- 3. aur_tome_step -> aur_tome_map_rows
def test_tome_step_indices_chain_to_the_definition_and_to_the_step_sizes(mid):
    gen = torch.Generator().manual_seed(5)
    frames, t0, c, d, r, layers = 2, 82, 16, 64, 6, 5
    x = torch.randn(frames, t0, d, generator=gen).half()
    size = None
    rows = dev(np.tile(np.arange(t0, dtype=np.int32), (frames, 1)))
    steps, t = [], t0
    for _ in range(layers):
        metric = torch.randn(frames, t, c, generator=gen)
        x, so, idx = mid.tome_step(metric, x, size, r)
        assert idx["r"] == r
        mid.tome_map_rows(rows, t, idx["r"], idx["unm_idx"], idx["src_idx"], idx["dst_idx"])
        steps.append(tuple(idx[k].cpu().numpy() for k in ("unm_idx", "src_idx", "dst_idx")))
        size, t = so[..., None], t - idx["r"]
    got = rows.cpu().numpy()
    np.testing.assert_array_equal(got, MM.compose(t0, steps))
    assert t == t0 - layers * r
    final = size[..., 0].cpu().numpy()
    for f in range(frames):
        np.testing.assert_array_equal(np.bincount(got[f], minlength=t).astype(np.float32), final[f])


# ---------------------------------------------------------------------------------------------- 4. aur_vit_encode_map
def _check_map(mp, sz, frames, gh, gw, n_kept):
    m, s = mp.cpu().numpy(), sz.cpu().numpy()
    assert m.shape == (frames, gh, gw) and m.dtype == np.int32 and s.shape == (frames, n_kept) and s.dtype == np.float32
    assert m.min() >= 0 and m.max() < n_kept
    for f in range(frames):
        np.testing.assert_array_equal(np.bincount(m[f].reshape(-1), minlength=n_kept).astype(np.float32), s[f])
    assert s.sum(axis=1).tolist() == [float(gh * gw)] * frames
    return m, s


@pytest.mark.parametrize("which,r", [("tiny", 2), ("mid", 15)])
def test_vit_encode_map_agrees_with_the_sizes_the_merge_kernels_build(tiny, mid, which, r):
    """What this proves: the WIRING of the map launch into the layer loop - it runs behind every merging layer, on that layer's
    indices and token count, before they are overwritten - because the map's bincount equals, exactly, the size vector the merge
    kernels build from the same indices, and the tokens stay bitwise those of aur_vit_encode_hw.  What it does not prove: the rule
    itself (a wrong rule applied consistently to map and to nothing else would still fail here only by luck of the bincount);
    tests 1 and 3 above hold the rule against the reference's merge_source and against aur_tome_step's own outputs."""
    eng, cfg = (tiny, VIT_TINY) if which == "tiny" else (mid, VIT_MID)
    side, g = cfg["image_size"], cfg["image_size"] // cfg["patch_size"]
    F = MAX_FRAMES[which]
    gen = torch.Generator().manual_seed(11)
    px = torch.randn(F, 3, side, side, generator=gen).half().cuda()
    px[F - 1] = px[0]                                                 # the same frame twice
    plain = eng.vit_encode(px, r)
    tok, mp, sz = eng.vit_encode(px, r, merge_map=True)
    n_kept = plain.shape[1]
    assert n_kept == g * g - r * (cfg["num_hidden_layers"] - 1)
    assert torch.equal(tok.view(torch.int16), plain.view(torch.int16))
    m, s = _check_map(mp, sz, F, g, g, n_kept)
    assert (s > 1).any()
    np.testing.assert_array_equal(m[F - 1], m[0])
    # two frames swapped: the two maps swapped;  one frame alone: its map
    tok2, mp2, sz2 = eng.vit_encode(px[[1, 0]].contiguous(), r, merge_map=True)
    np.testing.assert_array_equal(mp2.cpu().numpy(), m[[1, 0]])
    np.testing.assert_array_equal(sz2.cpu().numpy(), s[[1, 0]])
    assert torch.equal(tok2.view(torch.int16), plain[[1, 0]].view(torch.int16))
    tok1, mp1, sz1 = eng.vit_encode(px[1:2], r, merge_map=True)
    np.testing.assert_array_equal(mp1.cpu().numpy(), m[1:2])
    np.testing.assert_array_equal(sz1.cpu().numpy(), s[1:2])
    # the map really is where the patches went: unmerging the per-token patch count reproduces sizes[map]
    un = eng.unmerge(tok, mp)
    assert un.shape == (F, g, g, cfg["hidden_size"])
    assert torch.equal(un[0, 0, 0].view(torch.int16), tok[0, int(m[0, 0, 0])].view(torch.int16))
    # r = 0: the identity and ones
    tok0, mp0, sz0 = eng.vit_encode(px, 0, merge_map=True)
    assert torch.equal(tok0.view(torch.int16), eng.vit_encode(px, 0).view(torch.int16))
    np.testing.assert_array_equal(mp0.cpu().numpy(), np.tile(np.arange(g * g, dtype=np.int32).reshape(1, g, g), (F, 1, 1)))
    np.testing.assert_array_equal(sz0.cpu().numpy(), np.ones((F, g * g), np.float32))


def test_vit_encode_map_on_a_non_square_input(tiny):
    gen = torch.Generator().manual_seed(12)
    px = torch.randn(3, 3, 42, 70, generator=gen).half().cuda()       # a 3 x 5 grid through aur_vit_pos_interp: T0 = 16
    assert tiny.interpolated_pos(42, 70) is not None
    plain = tiny.vit_encode(px, 2)
    tok, mp, sz = tiny.vit_encode(px, 2, merge_map=True)
    assert torch.equal(tok.view(torch.int16), plain.view(torch.int16))
    _check_map(mp, sz, 3, 3, 5, 15 - 2 * 3)
    # a schedule that runs into the (t - 1) // 2 clamp at every layer: 16 -> 9 -> 5 -> 3 rows
    tokc, mpc, szc = tiny.vit_encode(px, 7, merge_map=True)
    assert tokc.shape[1] == 2
    _check_map(mpc, szc, 3, 3, 5, 2)


def test_vit_encode_map_recorded_in_a_graph_and_replayed(tiny):
    gen = torch.Generator().manual_seed(13)
    F, r = 2, 2
    inputs = [torch.randn(F, 3, 56, 56, generator=gen).half().cuda() for _ in range(2)]
    eager = [tuple(t.clone() for t in tiny.vit_encode(p, r, merge_map=True)) for p in inputs]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        px = torch.zeros_like(inputs[0])
        outs = (torch.zeros_like(eager[0][0]), torch.full_like(eager[0][1], -1), torch.zeros_like(eager[0][2]))
        run = lambda: tiny.vit_encode(px, r, out=outs, merge_map=True)
        run()
        gid, nodes = tiny.graph_capture(run)
        # the plain call's recording holds one node less per merging layer, and two less for the map's start and end
        gid0, nodes0 = tiny.graph_capture(lambda: tiny.vit_encode(px, r, out=outs[0]))
        assert nodes == nodes0 + (VIT_TINY["num_hidden_layers"] - 1) + 2
        try:
            for p, want in zip(inputs, eager):
                px.copy_(p)
                outs[1].fill_(-1)
                tiny.graph_launch(gid)
                st.synchronize()
                assert torch.equal(outs[0].view(torch.int16), want[0].view(torch.int16))
                assert torch.equal(outs[1], want[1]) and torch.equal(outs[2], want[2])
        finally:
            tiny.graph_destroy(gid)
            tiny.graph_destroy(gid0)
    assert not torch.equal(eager[0][1], eager[1][1])                  # two inputs, two maps


# ---------------------------------------------------------------------------------------------- 5. AuroraModel, inference.py
def test_model_forward_with_output_merge_map():
    from aurora_amd.model import AuroraModel
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_checkpoint_e2e.npz"))
    N = 8
    m = AuroraModel.from_pretrained(TINY, max_frames=4, max_batch=1, max_ctx=256, max_new_tokens=N)
    try:
        m.visual_encoder.reset_tome_r(float(g["ratio"]))
        px = torch.from_numpy(g["pixel_values"]).cuda()
        data = {"pixel_values": px.unsqueeze(0), "input_ids": torch.from_numpy(g["input_ids"])}
        plain = m(data, mode="inference")
        out = m(dict(data, output_merge_map=True), mode="inference")
        assert set(out) == set(plain) | {"merge_map", "merge_sizes"} and "merge_map" not in plain
        assert torch.equal(out["inputs_embeds"].view(torch.int16), plain["inputs_embeds"].view(torch.int16))
        ids = m.llm.generate(**plain, do_sample=False, num_beams=1, max_new_tokens=N, eos_token_id=None)
        assert torch.equal(m.llm.generate(**out, do_sample=False, num_beams=1, max_new_tokens=N, eos_token_id=None), ids)
        F, n_kept = px.shape[0], int(g["n_kept"])
        assert out["merge_map"].shape == (F, 4, 4) and out["merge_map"].dtype == torch.int32
        assert len(out["merge_sizes"]) == F and all(s.shape == (n_kept,) for s in out["merge_sizes"])
        _check_map(out["merge_map"], torch.stack(out["merge_sizes"]), F, 4, 4, n_kept)
    finally:
        m.engine.close()


def test_slowfast_frame_zero_carries_the_identity_map():
    from aurora_amd.model import AuroraModel
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_checkpoint_e2e.npz"))
    m = AuroraModel.from_pretrained(TINY, max_frames=4, max_batch=1, max_ctx=256, max_new_tokens=8, slowfast=True)
    try:
        px = torch.from_numpy(g["pixel_values"]).cuda()
        data = {"pixel_values": px.unsqueeze(0), "input_ids": torch.from_numpy(g["input_ids"])}
        m.visual_encoder.reset_tome_r(float(g["ratio"]))
        plain = m(data, mode="inference")
        m.visual_encoder.reset_tome_r(float(g["ratio"]))              # the slow-fast forward leaves the ratio at 1.0
        out = m(dict(data, output_merge_map=True), mode="inference")
        assert torch.equal(out["inputs_embeds"].view(torch.int16), plain["inputs_embeds"].view(torch.int16))
        mp, szs = out["merge_map"].cpu().numpy(), out["merge_sizes"]
        assert mp.shape == (3, 4, 4) and [len(s) for s in szs] == [16, int(g["n_kept"]), int(g["n_kept"])]
        np.testing.assert_array_equal(mp[0], np.arange(16, dtype=np.int32).reshape(4, 4))
        assert torch.equal(szs[0].cpu(), torch.ones(16))
        _check_map(out["merge_map"][1:], torch.stack(szs[1:]), 2, 4, 4, int(g["n_kept"]))
    finally:
        m.engine.close()


def test_cli_writes_the_map_and_the_picture_and_prints_the_same_caption(tmp_path):
    from PIL import Image
    from aurora_amd.model import AuroraModel
    from aurora_amd.preprocess import CLIP_MEAN, CLIP_STD, FramePreprocessor
    g = np.load(os.path.join(ROOT, "tests", "golden", "g14_cli_e2e.npz"))
    npz, png = str(tmp_path / "map.npz"), str(tmp_path / "map.png")
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--model_path", TINY, "--visual_input", os.path.join(TINY, "clip.png"),
           "--prompt", str(g["prompt"]), "--token_kept_ratio", str(float(g["ratio"])), "--max_new_tokens", str(int(g["new"]))]
    base = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert base.returncode == 0, base.stderr[-3000:]
    r = subprocess.run(cmd + ["--merge_map", npz, "--merge_vis", png], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == base.stdout and str(g["text"]) in r.stdout
    assert os.path.getsize(npz) > 0 and os.path.getsize(png) > 0
    z = np.load(npz)
    m = AuroraModel.from_pretrained(TINY, max_frames=1, max_batch=1, max_ctx=128, max_new_tokens=4)
    try:
        m.visual_encoder.reset_tome_r(float(g["ratio"]))
        image = np.asarray(Image.open(os.path.join(TINY, "clip.png")).convert("RGB"))
        px = FramePreprocessor(image=56)(torch.from_numpy(np.array(image[None])).cuda())
        _, mp, sz = m.visual_encoder(px, output_merge_map=True)
    finally:
        m.engine.close()
    np.testing.assert_array_equal(z["merge_map"], mp.cpu().numpy())
    np.testing.assert_array_equal(z["sizes"], sz.cpu().numpy())
    assert z["grid"].tolist() == [4, 4] and float(z["token_kept_ratio"]) == float(g["ratio"]) and z["n_kept"].tolist() == [sz.shape[1]]
    img = np.asarray(Image.open(png))
    assert img.shape == (56, 56, 3)
    # the picture shows the model's input frames: the normalised pixels back as 8-bit RGB, rendered by the definition
    rgb = px.float().cpu().numpy().transpose(0, 2, 3, 1) * np.asarray(CLIP_STD, np.float32) + np.asarray(CLIP_MEAN, np.float32)
    want = MM.render(np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8), z["merge_map"], 14)
    np.testing.assert_array_equal(img, want[0])

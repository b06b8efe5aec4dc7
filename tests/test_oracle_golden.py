"""Pin the oracle (oracle/aurora_oracle.py + oracle/tome_ref.c) against the golden vectors that
were produced by the reference's own modules (tests/golden/make_golden.py).  CPU only."""
import json

import numpy as np
import pytest
import torch

from oracle import aurora_oracle as O
from oracle import tome_ref
from tests.util import cfg_of, enc_layers, golden, sub, tt


def test_g1_schedule_table():
    tab = golden("g1_schedule.npz")["table"]
    for L, ratio, r, kept in tab:
        L = int(L)
        assert O.tome_r(378, 378, 14, float(ratio), L) == int(r)
        assert O.kept_tokens(378, 378, 14, float(ratio), L) == int(kept)
    # the SURVEY section-8 table (L=32): bold BASELINE configs
    assert O.kept_tokens(378, 378, 14, 0.3, 32) == 264
    assert O.kept_tokens(378, 378, 14, 0.2, 32) == 171
    assert O.kept_tokens(378, 378, 14, 0.8, 32) == 605
    assert O.tome_r(378, 378, 14, 0.8, 32) == 4      # 1-0.8 = 0.19999999999999996 in doubles


@pytest.mark.parametrize("r", [1, 2, 3, 5])
def test_g2_tome_kat(r):
    g = golden("g2_tome_kat.npz")
    metric, x = tt(g["metric"]), tt(g["x"])
    y, s, m = O.tome_step(metric, x, None, r)
    np.testing.assert_array_equal(y.numpy(), g[f"r{r}_y"])
    np.testing.assert_array_equal(s.numpy(), g[f"r{r}_size"])
    for k in ("unm_idx", "src_idx", "dst_idx"):
        np.testing.assert_array_equal(m[k].numpy(), g[f"r{r}_{k}"])
    # C oracle: same indices, same merged values
    mc = tome_ref.match(g["metric"], r)
    for k in ("unm_idx", "src_idx", "dst_idx"):
        np.testing.assert_array_equal(mc[k], g[f"r{r}_{k}"])
    yc, sc = tome_ref.merge(g["x"], np.ones((1, 9), np.float32), mc)
    np.testing.assert_array_equal(yc, g[f"r{r}_y"])
    np.testing.assert_array_equal(sc[..., None], g[f"r{r}_size"])


def test_g2_chain_and_g3_ties():
    g = golden("g2_tome_kat.npz")
    metric, x = tt(g["metric"]), tt(g["x"])
    y1, s1, _ = O.tome_step(metric, x, None, 2)
    y2, s2, _ = O.tome_step(y1, y1, s1, 2)
    np.testing.assert_allclose(y2.numpy(), g["chain_y"], rtol=1e-6)
    np.testing.assert_array_equal(s2.numpy(), g["chain_size"])
    # tie rule: first maximum for argmax, lowest index first for selection
    for impl in ("py", "c"):
        if impl == "py":
            m = O.bipartite_match(tt(g["tie_metric"]), 2)
            got = {k: m[k].numpy() for k in ("unm_idx", "src_idx", "dst_idx")}
        else:
            got = tome_ref.match(g["tie_metric"], 2)
        for k in ("unm_idx", "src_idx", "dst_idx"):
            np.testing.assert_array_equal(got[k], g[f"tie_{k}"], err_msg=f"{impl}:{k}")


@pytest.mark.parametrize("t,seed", [(730, 0), (265, 1), (606, 2)])
@pytest.mark.parametrize("r", [4, 15, 18, 22])
def test_g4_tome_path_shapes(t, seed, r):
    g = golden("g4_tome_shapes.npz")
    key = f"t{t}_r{r}"
    gen = torch.Generator().manual_seed(int(g[key + "_seed"]))
    metric = torch.randn(2, t, 80, generator=gen)
    assert g[key + "_gaps"][:2].min() > 2e-6          # fixture avoids near-ties
    m = O.bipartite_match(metric, r)
    mc = tome_ref.match(metric.numpy(), r)
    for k in ("unm_idx", "src_idx", "dst_idx"):
        np.testing.assert_array_equal(m[k].numpy(), g[f"{key}_{k}"], err_msg=k)
        np.testing.assert_array_equal(mc[k], g[f"{key}_{k}"], err_msg="C:" + k)


def test_g5_merge_wavg_sizes():
    g = golden("g5_merge_wavg.npz")
    metric, x, size = tt(g["metric"]), tt(g["x"]).float(), tt(g["size"])
    y, s, m = O.tome_step(metric, x, size, 15)
    np.testing.assert_array_equal(m["src_idx"].numpy(), g["src_idx"])
    np.testing.assert_allclose(y.numpy(), g["y"], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(s.numpy(), g["size_out"])
    mc = tome_ref.match(g["metric"], 15)
    yc, sc = tome_ref.merge(x.numpy(), g["size"][..., 0], mc)
    np.testing.assert_allclose(yc, g["y"], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(sc, g["size_out"][..., 0])


@pytest.mark.parametrize("tag", ["tiny", "hd80"])
def test_g6_attention(tag):
    g = golden("g6_attention.npz")
    lw = sub(g, f"{tag}.w.")
    x, size = tt(g[f"{tag}.x"]), tt(g[f"{tag}.size"])
    heads = int(g[f"{tag}.heads"])
    o, metric = O.vit_attention(x, None, lw, heads)
    np.testing.assert_allclose(o.numpy(), g[f"{tag}.out"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(metric.numpy(), g[f"{tag}.metric"], rtol=1e-5, atol=1e-6)
    o2, _ = O.vit_attention(x, size, lw, heads)
    np.testing.assert_allclose(o2.numpy(), g[f"{tag}.out_size"], rtol=1e-4, atol=2e-6)
    # the proportional-attention term is a softmax no-op
    assert np.abs(g[f"{tag}.out_size"] - g[f"{tag}.out"]).max() < 1e-5


@pytest.mark.parametrize("tag", ["tiny", "gelu"])
def test_g7_encoder_chain(tag):
    g = golden("g7_encoder.npz")
    cfg = cfg_of(g, f"{tag}.cfg")
    layers = enc_layers(sub(g, f"{tag}.w."), cfg["L"])
    hs = O.vit_encoder(tt(g[f"{tag}.x"]), layers, cfg["heads"], cfg["r"], cfg["act"])
    if tag == "tiny":
        assert [h.shape[1] for h in hs] == [17, 15, 13, 11, 9]
        for i, h in enumerate(hs):
            np.testing.assert_allclose(h.numpy(), g[f"tiny.hs{i}"], rtol=2e-4, atol=2e-5)
    else:
        np.testing.assert_allclose(hs[-1].numpy(), g["gelu.hs_last"], rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(hs[-2].numpy(), g["gelu.hs_m2"], rtol=2e-4, atol=2e-5)


def mid_encoder_weights(g):
    """Re-create the seeded weights of the g7 'mid' encoder (recipe in make_golden.py)."""
    cfg = cfg_of(g, "cfg")
    names = json.loads(str(g["names"]))
    D, inter = cfg["D"], cfg["inter"]
    shapes = {}
    for n in names:
        leaf = n.split(".", 2)[2]
        if leaf.endswith("weight"):
            if "fc1" in leaf:
                shapes[n] = (inter, D)
            elif "fc2" in leaf:
                shapes[n] = (D, inter)
            elif "layer_norm" in leaf:
                shapes[n] = (D,)
            else:
                shapes[n] = (D, D)
        else:
            shapes[n] = (inter,) if "fc1" in leaf else (D,)
    gen = torch.Generator().manual_seed(cfg["wseed"])
    flat = {}
    for n in names:
        if len(shapes[n]) == 2:
            flat[n] = torch.randn(shapes[n], generator=gen) * 0.05
    for n in names:
        if len(shapes[n]) == 1:
            if "layer_norm" in n and n.endswith("weight"):
                flat[n] = 1.0 + 0.1 * torch.randn(shapes[n], generator=gen)
            else:
                flat[n] = 0.02 * torch.randn(shapes[n], generator=gen)
    x = torch.randn(2, cfg["T"], D, generator=gen)
    return cfg, enc_layers(flat, cfg["L"]), x


def test_g7_encoder_mid_indices_and_rows():
    g = golden("g7_encoder_mid.npz")
    cfg, layers, x = mid_encoder_weights(g)
    cap = []
    hs = O.vit_encoder(x, layers, cfg["heads"], cfg["r"], cfg["act"], capture=cap)
    np.testing.assert_array_equal([h.shape[1] for h in hs], g["counts"])
    rows = np.array([0, 1, 2, 50, 100, 200, 264, -1])
    for li, c in enumerate(cap):
        for k in ("unm_idx", "src_idx", "dst_idx"):
            np.testing.assert_array_equal(c["match"][k].numpy(), g[f"l{li}_{k}"], err_msg=f"layer {li} {k}")
        # the C oracle agrees with the reference indices on the same metric
        mc = tome_ref.match(c["metric"].numpy(), cfg["r"])
        for k in ("unm_idx", "src_idx", "dst_idx"):
            np.testing.assert_array_equal(mc[k], g[f"l{li}_{k}"], err_msg=f"C layer {li} {k}")
    for i, h in enumerate(hs):
        np.testing.assert_allclose(h[:, rows].numpy(), g[f"hs{i}_rows"], rtol=1e-3, atol=1e-4)


def test_g8_projector_splice_and_constants():
    g = golden("g8_projector_splice.npz")
    pw = sub(g, "proj.")
    vis = O.projector(tt(g["vis_in"]), pw)
    np.testing.assert_allclose(vis.numpy(), g["vis"], rtol=1e-5, atol=1e-6)
    emb = O.splice(tt(g["ids"])[0], tt(g["embed"]), tt(g["vis"]).view(2, 5, 96))
    np.testing.assert_array_equal(emb.numpy(), g["inputs_embeds"][0])
    assert emb.shape[0] == 16
    assert str(g["vicuna_instruction"]) == O.VICUNA_INSTRUCTION
    assert int(g["image_token_index"]) == O.IMAGE_TOKEN_INDEX
    assert str(g["default_image_token"]) == O.DEFAULT_IMAGE_TOKEN


def llama_weights(g):
    flat = sub(g, "w.")
    cfg = cfg_of(g, "cfg")
    layers = []
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        layers.append({k[len(p):].replace("self_attn.", "").replace("mlp.", ""): v
                       for k, v in flat.items() if k.startswith(p)})
    lw = dict(layers=layers)
    lw["norm.weight"] = flat["model.norm.weight"]
    lw["embed_tokens.weight"] = flat["model.embed_tokens.weight"]
    lw["lm_head.weight"] = flat["lm_head.weight"]
    return lw, cfg


def test_g9_llama_greedy_and_logits():
    g = golden("g9_llama_tiny.npz")
    lw, cfg = llama_weights(g)
    ids, logits = O.llama_greedy(tt(g["embeds"])[0], lw, cfg, 8, eos_id=None, return_logits=True)
    np.testing.assert_array_equal(ids, g["ids"][0])
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=1e-3, atol=2e-4)


def test_g9b_llama_head_dim_128_at_long_positions():
    """G9b (VERDICT r5 next #7 ii): HF LlamaForCausalLM - the model inference.py:47-51 decodes with - at the path's head_dim (128) and
    positions (prefill rows around 2100, the long-KV config's 6.9 k) under linear RoPE scaling x4.  The oracle's prefill form must
    reproduce HF's logits at every kept row, and its KV-cache form (prefill 6850 positions, then one position per call, as generate
    does) must reproduce the last 24 - the form the 7B-width GPU tests compare the kernels with."""
    g = golden("g9b_llama_hd128_long.npz")
    lw, cfg = llama_weights(g)
    lw = {k: (v.float() if torch.is_tensor(v) else [{kk: vv.float() for kk, vv in l.items()} for l in v]) for k, v in lw.items()}
    assert cfg["hidden_size"] // cfg["num_attention_heads"] == 128 and cfg["rope_factor"] == 4.0
    ids = tt(g["ids"]).long()
    rows = g["rows"].tolist()
    assert rows[-1] == len(ids) - 1 == 6873
    x = lw["embed_tokens.weight"][ids]
    h, _ = O.llama_forward(x, lw, cfg, None, 0)
    logits = torch.nn.functional.linear(h[rows], lw["lm_head.weight"])
    scale = float(np.abs(g["logits"]).max())
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=1e-3, atol=2e-4 * scale)
    # KV-cache form at long positions
    h0, kv = O.llama_forward(x[:6850], lw, cfg, None, 0)
    step = []
    for t in range(6850, 6874):
        ht, kv = O.llama_forward(x[t:t + 1], lw, cfg, kv, t)
        step.append(torch.nn.functional.linear(ht, lw["lm_head.weight"])[0])
    np.testing.assert_allclose(torch.stack(step).numpy(), g["logits"][16:], rtol=1e-3, atol=2e-4 * scale)
    # a restatement with the wrong scaling or the interleaved rotation would be far outside these bounds: the rows are sensitive to RoPE
    bad = dict(cfg, rope_factor=1.0)
    hb, _ = O.llama_forward(x[:2108], lw, bad, None, 0)
    lb = torch.nn.functional.linear(hb[rows[8:16]], lw["lm_head.weight"]).numpy()
    assert np.abs(lb - g["logits"][8:16]).max() > 20 * 2e-4 * scale


def test_process_text_and_prompt():
    text = O.build_prompt("Describe the video in detail.", 3)
    assert text == "USER: <image> <image> <image>\nDescribe the video in detail. ASSISTANT:"
    enc = lambda s, special: ([1] if special else []) + [100 + len(s)]
    ids = O.process_text(text, enc)
    assert ids == [1, 106, -200, 101, -200, 101, -200, 141]


# ---------------------------------------------------------------------------------------------------
# G17: trained-checkpoint statistics (tests/golden/make_golden_ckpt_stats.py).  The fixture is the yardstick of
# tests/test_gpu_ckpt_stats.py - HF's own fp16 error against an fp64 evaluation - so what is pinned here is the yardstick itself:
# the generators reproduce the hashed tensors, the oracle reproduces the fp64 logits, the yardstick is tight and finite, and the
# cases leave the greedy-id comparison something to compare.
# ---------------------------------------------------------------------------------------------------
def _g17_sha(tensors):
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.half().numpy()).tobytes())
    return h.hexdigest()


def _g17_llm_tensors(w):
    out = [w["embed_tokens.weight"], w["norm.weight"], w["lm_head.weight"]]
    for lw in w["layers"]:
        out += [lw[k] for k in sorted(lw)]
    return out


def _g17_names():
    from tests.util import ckpt_llm_cases
    return [c[0] for c in ckpt_llm_cases()]


def test_g17_covers_the_cases_of_the_issue():
    from tests.util import CKPT_PREFIX_LENGTHS, ckpt_llm_cases
    cases = {(s, g, e, T) for _, s, g, e, T in ckpt_llm_cases()}
    assert tuple(CKPT_PREFIX_LENGTHS) == (40, 97, 300)
    for seed in (0, 1):
        for T in (40, 97, 300):
            for gain, scales in ((1.0, (1.0, 2.0 ** -6, 2.0 ** -10, 2.0 ** 6)), (3.0, (1.0, 2.0 ** -6))):
                for sc in scales:
                    assert (seed, gain, sc, T) in cases
    assert {(5, 8.0, 1.0, 300), (5, 8.0, 1.0, 97), (4, 8.0, 2.0 ** -6, 97)} <= cases    # the sharp-softmax cases that stay inside the cap
    g = golden("g17_ckpt_stats.npz")
    for name in _g17_names():
        assert f"llm.{name}.logits" in g.files, name


@pytest.mark.parametrize("name", _g17_names())
def test_g17_generators_oracle_and_yardstick(name):
    from tests.util import CKPT_LLM_CFG as cfg, CKPT_NEW_TOKENS, ckpt_like_llm_case, ckpt_llm_cases, ckpt_stored_rows
    g = golden("g17_ckpt_stats.npz")
    _, seed, gain, scale, T = next(c for c in ckpt_llm_cases() if c[0] == name)
    p = f"llm.{name}."
    w, emb = ckpt_like_llm_case(cfg, seed, gain, scale, T)
    # every tensor fp16-representable, and the ones the fixture was made from
    for t in _g17_llm_tensors(w) + [emb]:
        assert torch.equal(t, t.half().float()) and torch.isfinite(t).all()
    assert _g17_sha(_g17_llm_tensors(w)) == str(g[p + "sha_w"]), "ckpt_like_llm_weights drifted from the fixture (RNG?)"
    assert _g17_sha([emb]) == str(g[p + "sha_x"]), "ckpt_like_embeds drifted from the fixture (RNG?)"
    rows, ids, ref = g[p + "rows"].astype(np.int64), g[p + "ids"].astype(np.int64), tt(g[p + "logits"]).double()
    lscale = float(g[p + "scale"])
    assert list(rows) == ckpt_stored_rows(T) and len(ids) == CKPT_NEW_TOKENS
    for k in ("logits", "margin", "hf32", "hf16", "scale"):
        assert np.isfinite(g[p + k]).all(), k
    assert g[p + "margin"].shape == g[p + "hf16"].shape == g[p + "hf32"].shape == (T + CKPT_NEW_TOKENS - 1,)
    assert np.abs(g[p + "logits"]).max() <= lscale * (1 + 1e-6)                  # the scale is the maximum over ALL rows, stored or not
    # the oracle in fp32 on these statistics: 1e-5 of the logit scale from the fp64 evaluation (measured ~1e-6)
    full = torch.cat([emb, w["embed_tokens.weight"][tt(ids[:-1])]], 0)
    h, _ = O.llama_forward(full, w, cfg, None, 0)
    got = torch.nn.functional.linear(h, w["lm_head.weight"])
    err = (got[rows].double() - ref).abs().max().item() / lscale
    assert err <= 1e-5, err
    top2 = got.double().topk(2, dim=1).values
    np.testing.assert_allclose((top2[:, 0] - top2[:, 1]).numpy(), g[p + "margin"], atol=4e-5 * lscale)
    for j in range(CKPT_NEW_TOKENS):                     # the ids are the fp64 greedy choice, reproduced wherever fp32 can tell
        if g[p + "margin"][T - 1 + j] > 4e-5 * lscale:
            assert int(got[T - 1 + j].argmax()) == ids[j], j
    # HF in fp32 is the same function (so HF in fp16 is a yardstick for it), and the yardstick is inside its cap
    assert float(g[p + "hf32"].max()) <= 1e-5, float(g[p + "hf32"].max())
    worst16 = float(g[p + "hf16"].max())
    assert float(g["cap"]) == 5e-3 and worst16 <= 5e-3, worst16
    assert worst16 >= 2.0 ** -13                         # ... and is an fp16 error, not an accident of zeros
    # the id comparison on the GPU is not vacuous: >= 90 % of the prefix rows have a margin above twice the case's HF-fp16 error
    clear = int((g[p + "margin"][:T] > 2 * worst16 * lscale).sum())
    assert clear >= 0.9 * T, (clear, T)


@pytest.mark.parametrize("name", ["hd80_gelu", "hd16_quick"])
def test_g17_vit_layer_generators_and_oracle(name):
    from tests.util import CKPT_VIT_CASES, ckpt_like_vit_input, ckpt_like_vit_weights, rel_l2
    g = golden("g17_ckpt_stats.npz")
    cfg, frames, r, wseed, xseed = CKPT_VIT_CASES[name]
    p = f"vit.{name}."
    t = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    lw = ckpt_like_vit_weights(cfg, wseed)["layers"][0]
    x = ckpt_like_vit_input(xseed, frames, t, cfg["hidden_size"])
    for v in list(lw.values()) + [x]:
        assert torch.equal(v, v.half().float())
    assert _g17_sha([lw[k] for k in sorted(lw)]) == str(g[p + "sha_w"])
    assert _g17_sha([x]) == str(g[p + "sha_x"])
    assert cfg["hidden_size"] // cfg["num_attention_heads"] in (80, 16)
    match = dict(r=r, **{k: tt(g[p + k].astype(np.int64)) for k in ("unm_idx", "src_idx", "dst_idx")})
    out, size = O.vit_layer(x, None, lw, cfg["num_attention_heads"], r, cfg["hidden_act"], forced_match=match)
    assert rel_l2(out, tt(g[p + "out"])) <= 1e-5
    np.testing.assert_array_equal(size[..., 0].numpy(), g[p + "size"])
    assert "AuroraCLIPEncoderLayer" in str(g["vit_reference_module"])
    r16, r32 = float(g[p + "ref16_rel_l2"]), float(g[p + "ref32_rel_l2"])
    assert np.isfinite([r16, r32]).all() and r32 <= 1e-5 and 2.0 ** -13 <= r16 <= 5e-3, (r16, r32)

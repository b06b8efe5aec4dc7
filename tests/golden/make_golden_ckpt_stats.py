#!/usr/bin/env python3
"""G17: the yardstick for the kernels under trained-checkpoint statistics (tests/util.py `ckpt_like_*`): on the SAME realistic
inputs, how far the reference's own fp16 arithmetic is from an fp64 evaluation.

The reference runs its models with `torch_dtype=torch.float16` (inference.py:50,54), so its own half-precision error is a bound that
does not come from the code under test: tests/test_gpu_ckpt_stats.py holds the HIP path to 1.5x of it.

Llama (HF `LlamaForCausalLM`, the decode model of the path; cfg tests.util.CKPT_LLM_CFG), per case of tests.util.ckpt_llm_cases():
  * sha256 of the generated weights and prefix (RNG drift guard),
  * `oracle.aurora_oracle.llama_forward` in fp64 over the prefix and the 15 fed-back greedy tokens (16 new ids, fp64's own choice):
    logits at tests.util.ckpt_stored_rows (kept as fp32 - 6e-8 relative, three orders below anything compared - and sampled, so that
    the committed file stays below 1 MiB), the top-1 / top-2 margin at EVERY row,
  * per row, max |HF - fp64| / max |fp64 logit of the case| for HF in fp32 and in fp16; the decode positions through HF's own
    KV-cache path (prefill on inputs_embeds, then one id per call), the prefix rows from that prefill.
The ViT part: one `AuroraCLIPEncoderLayer` of the reference (imported at generation time as make_golden.py does) per
tests.util.CKPT_VIT_CASES, in fp64-oracle vs reference-in-fp16 form, the merge forced to the fp64 oracle's indices.

CAP: a loose yardstick would hide a failure: a case whose worst HF-fp16 row is above 5e-3 of the logit scale is refused here
(and tests/test_oracle_golden.py asserts the same on the committed file).

Re-run:  python tests/golden/make_golden_ckpt_stats.py     (CPU, ~20 s; needs transformers and, for the ViT part, the reference tree)
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import aurora_oracle as O                                                               # noqa: E402
from tests import util as U                                                                         # noqa: E402

CAP = 5e-3


def sha_of(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.half().numpy()).tobytes())
    return h.hexdigest()


def llm_tensor_list(w):
    out = [w["embed_tokens.weight"], w["norm.weight"], w["lm_head.weight"]]
    for lw in w["layers"]:
        out += [lw[k] for k in sorted(lw)]
    return out


def to_double(w):
    return {k: ([{n: t.double() for n, t in lw.items()} for lw in v] if k == "layers" else v.double()) for k, v in w.items()}


def hf_model(w, cfg, dtype):
    from transformers import LlamaConfig, LlamaForCausalLM
    lcfg = dict(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                num_key_value_heads=cfg["num_attention_heads"], max_position_embeddings=16384, rms_norm_eps=cfg["rms_norm_eps"],
                rope_theta=cfg["rope_theta"], bos_token_id=1, eos_token_id=2, pad_token_id=0, tie_word_embeddings=False)
    try:
        c = LlamaConfig(**lcfg, rope_scaling={"type": "linear", "factor": cfg["rope_factor"]})
    except Exception:
        c = LlamaConfig(**lcfg, rope_scaling={"rope_type": "linear", "factor": cfg["rope_factor"]})
    m = LlamaForCausalLM(c).eval()
    sd = {"model.embed_tokens.weight": w["embed_tokens.weight"], "model.norm.weight": w["norm.weight"], "lm_head.weight": w["lm_head.weight"]}
    for i, lw in enumerate(w["layers"]):
        for k, v in lw.items():
            grp = "self_attn." if k[0] in "qkvo" and "_proj" in k else ("mlp." if "_proj" in k else "")
            sd[f"model.layers.{i}.{grp}{k}"] = v
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    return m.to(dtype)


def hf_rows(model, emb, ids, dtype):
    """logits [T + 15, V] (fp64 copy): prefix rows from the prefill on inputs_embeds, decode rows one id per call through the cache"""
    with torch.no_grad():
        out = model(inputs_embeds=emb[None].to(dtype), use_cache=True)
        rows, past = [out.logits[0].double()], out.past_key_values
        for t in ids[:-1]:
            o = model(input_ids=torch.tensor([[t]]), past_key_values=past, use_cache=True)
            past = o.past_key_values
            rows.append(o.logits[0].double())
    return torch.cat(rows, 0)


def llm_case(cfg, seed, gain, scale, T):
    w, emb = U.ckpt_like_llm_case(cfg, seed, gain, scale, T)
    wd = to_double(w)
    ids, _ = O.llama_greedy(emb.double(), wd, cfg, U.CKPT_NEW_TOKENS, eos_id=None, return_logits=True)
    full = torch.cat([emb, w["embed_tokens.weight"][torch.tensor(ids[:-1])]], 0)
    h, _ = O.llama_forward(full.double(), wd, cfg, None, 0)
    ref = torch.nn.functional.linear(h, wd["lm_head.weight"])                         # [T + 15, V] fp64
    assert [int(ref[T - 1 + j].argmax()) for j in range(U.CKPT_NEW_TOKENS)] == ids
    scale_l = ref.abs().max().item()
    errs = {}
    for tag, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
        got = hf_rows(hf_model(w, cfg, dt), emb, ids, dt)
        assert torch.isfinite(got).all(), (tag, "HF logits not finite")
        errs[tag] = ((got - ref).abs().amax(1) / scale_l).numpy().astype(np.float32)
    top2 = ref.topk(2, dim=1).values
    rows = U.ckpt_stored_rows(T)
    return dict(sha_w=sha_of(llm_tensor_list(w)), sha_x=sha_of([emb]), ids=np.asarray(ids, np.int16), rows=np.asarray(rows, np.int16),
                logits=ref[rows].numpy().astype(np.float32), scale=np.float64(scale_l),
                margin=(top2[:, 0] - top2[:, 1]).numpy().astype(np.float32), hf32=errs["fp32"], hf16=errs["fp16"])


def vit_case(R, name):
    from transformers.models.clip.configuration_clip import CLIPVisionConfig
    cfg, frames, r, wseed, xseed = U.CKPT_VIT_CASES[name]
    D, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    t = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    w = U.ckpt_like_vit_weights(cfg, wseed)
    x = U.ckpt_like_vit_input(xseed, frames, t, D)
    lw = w["layers"][0]
    lwd = {k: v.double() for k, v in lw.items()}
    cap = []
    ref, size = O.vit_layer(x.double(), None, lwd, heads, r, cfg["hidden_act"], capture=cap)
    match = cap[0]["match"]
    aurora, tome = R["aurora"], R["tome"]
    layer = aurora.AuroraCLIPEncoderLayer(CLIPVisionConfig(hidden_size=D, num_attention_heads=heads, num_hidden_layers=1,
                                                           intermediate_size=cfg["intermediate_size"], hidden_act=cfg["hidden_act"],
                                                           image_size=cfg["image_size"], patch_size=14, attention_dropout=0.0)).eval()
    sd = {}
    for k, v in lw.items():
        grp = "self_attn." if "_proj" in k else ("mlp." if k.startswith("fc") else "")
        sd[grp + k] = v
    layer.load_state_dict(sd, strict=True)
    orig = tome.bipartite_soft_matching
    seen = []

    def forced(metric, r, class_token=False, distill_token=False):
        # the merge of the fp64 oracle's metric, whatever the module's own (fp32 / fp16) metric would have chosen
        merge, un = orig(cap[0]["metric"].to(metric.dtype) if metric.dtype == torch.float64 else cap[0]["metric"].float(), r, class_token, distill_token)
        cells = dict(zip(merge.__code__.co_freevars, [c.cell_contents for c in merge.__closure__]))
        for k in ("unm_idx", "src_idx", "dst_idx"):
            assert torch.equal(cells[k][..., 0], match[k]), ("forced indices differ from the fp64 oracle's", k)
        seen.append(1)
        return merge, un

    aurora.bipartite_soft_matching = forced
    res = {}
    try:
        for tag, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
            with torch.no_grad():
                (out,), _ = layer.to(dt)(x.to(dt), r, None, None, None)
            assert out.dtype == dt and torch.isfinite(out).all()
            res[tag] = U.rel_l2(out.double(), ref)
    finally:
        aurora.bipartite_soft_matching = orig
    assert len(seen) == 2
    return dict(sha_w=sha_of([lw[k] for k in sorted(lw)]), sha_x=sha_of([x]), out=ref.numpy().astype(np.float32),
                size=size[..., 0].numpy().astype(np.float32), ref32_rel_l2=np.float64(res["fp32"]), ref16_rel_l2=np.float64(res["fp16"]),
                **{k: match[k].numpy().astype(np.int16) for k in ("unm_idx", "src_idx", "dst_idx")})


def main():
    import transformers
    torch.set_num_threads(4)              # a fixed count: the fp16 CPU sums (and so the recorded errors) depend on it
    fx, summary = {}, {}
    for name, seed, gain, scale, T in U.ckpt_llm_cases():
        c = llm_case(U.CKPT_LLM_CFG, seed, gain, scale, T)
        worst = float(c["hf16"].max())
        print(f"{name}: HF fp16 worst {worst:.2e}  HF fp32 worst {float(c['hf32'].max()):.1e}  logit scale {float(c['scale']):.3g}  "
              f"rows with margin > 2 x fp16 error {int((c['margin'][:T] > 2 * worst * c['scale']).sum())}/{T}", flush=True)
        if not worst <= CAP:
            raise SystemExit(f"{name}: the yardstick itself is at {worst:.2e} > {CAP}: refuse to write it (choose another seed; never raise the cap)")
        summary[name] = worst
        for k, v in c.items():
            fx[f"llm.{name}.{k}"] = np.array(v) if isinstance(v, str) else v
    sys.path.insert(0, HERE)
    from make_golden import import_reference
    R = import_reference()
    for name in U.CKPT_VIT_CASES:
        c = vit_case(R, name)
        print(f"vit {name}: reference fp16 rel-L2 {float(c['ref16_rel_l2']):.2e}  fp32 {float(c['ref32_rel_l2']):.1e}", flush=True)
        for k, v in c.items():
            fx[f"vit.{name}.{k}"] = np.array(v) if isinstance(v, str) else v
    fx["vit_reference_module"] = np.array("AuroraCLIPEncoderLayer of the reference (aurora.py:703-759) run in torch.float16 on the CPU; "
                                          "its bipartite_soft_matching given the fp64 oracle's metric (indices asserted equal)")
    fx["cap"] = np.float64(CAP)
    fx["versions"] = np.array(json.dumps({"torch": torch.__version__, "transformers": transformers.__version__, "numpy": np.__version__,
                                          "reference_pins": "transformers>=4.36.0,!=4.38.0-2,<=4.42.4 (src/xtuner/requirements/runtime.txt:26)"}))
    path = os.path.join(HERE, "g17_ckpt_stats.npz")
    np.savez_compressed(path, **fx)
    payload = hashlib.sha256()
    for k in sorted(fx):
        payload.update(k.encode() + np.ascontiguousarray(fx[k]).tobytes())
    print(path, os.path.getsize(path), "bytes; payload sha256", payload.hexdigest())
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()

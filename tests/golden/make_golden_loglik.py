#!/usr/bin/env python3
"""G19: the log-likelihood of a given continuation, as HF computes it - what the reference adaptor's `loglikelihood` intends
(lmms_eval/models/auroracap.py:232-297: one forward over context + continuation with `labels` masked to -100 over the context, the
loss over the continuation tokens, `logits.argmax(-1)` against them).

A tiny seeded `LlamaForCausalLM` in fp32 (weights fp16-representable, stored as fp16) and 3 cases:
  0  a continuation that IS the model's greedy continuation of its context                     -> is_greedy True
  1  a random continuation (most of its tokens are not the argmax of their rows)               -> is_greedy False
  2  case 0's greedy continuation with one token in the middle replaced by a non-argmax token  -> is_greedy False
Per case the fixture keeps the full ids, the labels HF was given, the context length, HF's `loss`, its `logits.argmax(-1)`, the per-token
log-probabilities (log_softmax of HF's logits at the rows that predict the continuation, gathered at the continuation tokens) and those
logits rows themselves.  `aurora_amd/scoring.py` on the rows, and `oracle.aurora_oracle.llama_forward` + lm_head on the weights, must give
-sum_logprob / n == loss and the same greedy flag (tests/test_scoring_host.py).

Third-party arithmetic: transformers (container: 5.15.0; the reference pins <= 4.42.4 - drift recorded in `versions`).
Re-run:  python tests/golden/make_golden_loglik.py      (CPU, seconds; needs transformers, not /root/reference)
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(21, 7), (34, 12), (21, 7)]              # (context tokens, continuation tokens)


def main():
    import transformers
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(1919)
    lcfg = dict(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=4, max_position_embeddings=256, rms_norm_eps=1e-5, rope_theta=1e4, bos_token_id=1,
                eos_token_id=2, pad_token_id=0, tie_word_embeddings=False)
    model = LlamaForCausalLM(LlamaConfig(**lcfg)).float().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            elif "embed_tokens" in n:
                p.copy_(torch.randn_like(p))
            elif "lm_head" in n:
                p.copy_(torch.randn_like(p) * (3.0 / p.shape[1] ** 0.5))      # logits of a few units: a peaked but not one-hot softmax
            else:
                p.copy_(torch.randn_like(p) * (0.6 / p.shape[1] ** 0.5))
            p.copy_(p.half().float())                                          # fp16-representable: the fixture stores fp16, nothing is lost
    g = torch.Generator().manual_seed(19)
    fx = {f"w.{k}": v.detach().half().numpy() for k, v in model.state_dict().items() if "rotary" not in k and "inv_freq" not in k}
    greedy0 = None
    for c, (lc, n) in enumerate(CASES):
        ctx = torch.randint(3, lcfg["vocab_size"], (lc,), generator=g) if c != 2 else ctx0
        if c in (0, 2):
            if greedy0 is None:
                ids = ctx.clone()
                with torch.no_grad():
                    for _ in range(n):                                         # greedy, one full forward per token: no cache, no generate()
                        nxt = model(input_ids=ids[None]).logits[0, -1].argmax()
                        ids = torch.cat([ids, nxt[None]])
                ctx0, greedy0 = ctx, ids[lc:]
            cont = greedy0.clone()
            if c == 2:
                with torch.no_grad():
                    row = model(input_ids=torch.cat([ctx, cont])[None]).logits[0, lc - 1 + 3]
                cont[3] = row.argsort(descending=True)[5]                      # the sixth most likely token at that row
        else:
            cont = torch.randint(3, lcfg["vocab_size"], (n,), generator=g)
        ids = torch.cat([ctx, cont])
        labels = ids.clone()
        labels[:lc] = -100                                                     # auroracap.py:276-278
        with torch.no_grad():
            out = model(input_ids=ids[None], labels=labels[None])
        logits = out.logits[0].float()
        rows = logits[lc - 1: lc - 1 + n]                                      # position lc - 1 + j predicts cont[j]
        lps = torch.log_softmax(rows.double(), -1).gather(1, cont[:, None])[:, 0]
        am = logits.argmax(-1)
        top2 = rows.topk(2, -1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3                   # no near-tie: the argmax is not a rounding matter
        flag = bool((am[lc - 1: lc - 1 + n] == cont).all())
        assert flag == (c == 0), (c, flag)
        assert abs(float(out.loss) + float(lps.sum()) / n) < 1e-5
        fx.update({f"c{c}.ids": ids.numpy().astype(np.int32), f"c{c}.labels": labels.numpy().astype(np.int32), f"c{c}.ctx_len": np.int32(lc),
                   f"c{c}.loss": np.float64(float(out.loss)), f"c{c}.argmax": am.numpy().astype(np.int32),
                   f"c{c}.token_logprobs": lps.numpy(), f"c{c}.rows": rows.numpy(), f"c{c}.greedy": np.bool_(flag)})
    fx.update(ncases=np.int32(len(CASES)), cfg=np.array(json.dumps(dict(lcfg, rope_factor=1.0))),
              versions=np.array(json.dumps({"torch": torch.__version__, "transformers": transformers.__version__,
                                            "reference_pins": "transformers>=4.36.0,!=4.38.0-2,<=4.42.4 (src/xtuner/requirements/runtime.txt:26)"})))
    path = os.path.join(HERE, "g19_loglik.npz")
    np.savez(path, **fx)
    print(path, os.path.getsize(path) / 1e6, "MB; losses", [float(fx[f"c{c}.loss"]) for c in range(len(CASES))])


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Where the ids of `tools/gpu/shared_prefix_stream.py` stop being reproducible (a tool, not a test).

    python tools/gpu/shared_prefix_diag.py [--out profiles/shared_prefix_diag.json]

The sharing engine of that tool ALONE (synthetic.AURORACAP_7B, 8 slots, 4 spare KV sequences + 1 holder, the same 16 clips x 5 prompts),
its KV pool zeroed once before the first pass.  On that one engine, in order:
  `unshared`            the stream without keys, three passes; the first is the reference of every comparison below;
  `shared`              the stream with `share_key`, three passes;
  `shared, serialised`  the same with the device idle before every prefix copy and after every sibling's staged prefill, three passes:
                        no sibling front end overlaps anything on another stream.
Per pass: how many of the 80 requests differ from the reference, (request, first differing token) for each, and how many K / V values
of the pool are not finite afterwards.  The file records; it decides nothing (exit status 0 unless a pass is incomplete).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES, RATIO, NEW, SLOTS, SPARE, BUCKET = 8, 0.3, 32, 8, 4, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix_diag.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--prompts", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine, splice_rows, tokens_at_layer, tome_r

    cfg = S.AURORACAP_7B
    v, l = cfg["vit"], cfg["llm"]
    r = tome_r(v["image_size"], v["image_size"], v["patch_size"], RATIO, v["num_hidden_layers"])
    n_kept = tokens_at_layer((v["image_size"] // v["patch_size"]) ** 2 + 1, r, v["num_hidden_layers"] - 1) - 1
    frames = [S.frames(FRAMES, i) for i in range(args.clips)]
    reqs, keys = [], []
    for i in range(args.clips):                                            # the requests of shared_prefix_stream.py
        ids0 = S.prompt_ids(FRAMES, i)
        head = ids0[:len(ids0) - ids0[::-1].index(-200)]
        for q in range(args.prompts):
            reqs.append((frames[i], head + np.random.default_rng(5000 + q).integers(3, l["vocab_size"], size=12 + 9 * q).tolist()))
            keys.append(i)
    lens = [splice_rows(ids, FRAMES, n_kept)["seq_len"] for _, ids in reqs]
    w = {"vit": S.vit_weights(v), "projector": S.projector_weights(v["hidden_size"], l["hidden_size"]), "llm": S.llm_weights(l)}
    e = AuroraCapEngine(cfg, w, max_frames=FRAMES, max_batch=SLOTS, max_ctx=max(lens) + 128 + NEW, max_new_tokens=NEW, prompt_bucket=BUCKET,
                        spare_slots=SPARE + 1, prefix_cache=1)
    del w
    torch.cuda.set_stream(e.stream)
    e.kv.zero_()

    def nonfinite():
        kv, bad, step = e.kv.view(torch.float16), 0, 1 << 30
        for o in range(0, kv.numel(), step):
            bad += int((~torch.isfinite(kv[o:o + step])).sum())
        return bad

    rows, ref = [], None

    def one_pass(variant, **kw):
        nonlocal ref
        torch.cuda.synchronize()
        got = dict(e.caption_stream(reqs, RATIO, NEW, eos_id=None, slots=SLOTS, overlap=True, **kw))
        torch.cuda.synchronize()
        if ref is None:
            ref = got
        diff = [(k, next((t for t, (x, y) in enumerate(zip(got.get(k, []), ref[k])) if x != y), -1)) for k in sorted(ref) if got.get(k) != ref[k]]
        rows.append(dict(variant=variant, complete=len(got) == len(reqs), requests_differing=len(diff), first_differences=diff,
                         nonfinite_kv_values=nonfinite()))
        print(json.dumps(rows[-1]), flush=True)

    share = dict(share_key=lambda k: keys[k])
    for _ in range(args.passes):
        one_pass("unshared")
    for _ in range(args.passes):
        one_pass("shared", **share)
    stage, copy = e.extend_stage, e.kv_copy_prefix
    e.extend_stage = lambda *a: (stage(*a), torch.cuda.synchronize())[0]
    e.kv_copy_prefix = lambda *a: (torch.cuda.synchronize(), copy(*a))[1]
    for _ in range(args.passes):
        one_pass("shared, serialised", **share)
    out = dict(model="synthetic.AURORACAP_7B", frames=FRAMES, token_kept_ratio=RATIO, max_new_tokens=NEW, slots=SLOTS, spare_sequences=SPARE,
               holders=1, prompt_bucket=BUCKET, requests=len(reqs), prompt_positions=[min(lens), max(lens)], kv_pool_values=e.kv.numel() // 2,
               reference="the first unshared pass (KV pool zeroed before it)", device=torch.cuda.get_device_name(0), passes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    e.close()
    return 0 if all(x["complete"] for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())

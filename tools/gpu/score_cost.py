#!/usr/bin/env python3
"""What scoring given continuations costs, shared against unshared (a tool, not a test).

    timeout -k 10 900 python tools/gpu/score_cost.py [--out profiles/score_cost.json] [--clips 16] [--passes 3] [--iters 200]

One process, synthetic weights at AuroraCap-7B shapes, 8 frames per clip, token_kept_ratio 0.3:

  * `batch`: `loglikelihood_batch` over `--clips` clips x 4 continuations of 16 tokens each (a multiple-choice task: one context per
    clip), on an engine of 8 KV sequences; the shared arm (`share=True`: one ViT pass per clip, the siblings copy the common pages
    and are scored behind the fork) and the unshared arm alternate, one warm-up pass each, then `--passes` timed passes each (wall
    time around the call, which synchronises at the end of every chunk); both arms' results are compared for equality;
  * `rows`: microseconds per launch of `score_rows_kernel` alone (aur_score_rows) on rows shaped like a language model's (N(0, 4^2)
    with 8 boosted tokens), 8 and 128 rows x 32000, from device events over `--iters` launches, three rounds.

No threshold hangs on the output; DESIGN section 5 quotes this file only.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_cost.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine

    frames, ratio, ncont, ntok, V = 8, 0.3, 4, 16, 32000
    cfg = S.AURORACAP_7B
    w = {"vit": S.vit_weights(cfg["vit"]), "projector": S.projector_weights(1280, 4096), "llm": S.llm_weights(cfg["llm"])}
    e = AuroraCapEngine(cfg, w, max_frames=frames, max_batch=8, max_ctx=64 + frames * 729 + ntok, max_new_tokens=16)
    out = dict(device=torch.cuda.get_device_name(0), frames=frames, token_kept_ratio=ratio, clips=args.clips, continuations=ncont,
               continuation_tokens=ntok, max_batch=8, batch=[], rows=[])
    items = []
    for c in range(args.clips):
        px, ctx = S.frames(frames, c), S.prompt_ids(frames, c)
        g = np.random.default_rng(5000 + c)
        items += [(px, ctx, g.integers(3, V, size=ntok).tolist()) for _ in range(ncont)]
    results = {}
    for rnd in range(-1, args.passes):                                      # round -1: warm-up, not recorded
        for share in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = e.loglikelihood_batch(items, ratio, share=share)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            results[share] = [(r["token_logprobs"], r["greedy"]) for r in res]
            if rnd >= 0:
                row = dict(round=rnd, share=share, seconds=round(dt, 4), ms_per_continuation=round(dt * 1e3 / len(items), 3))
                out["batch"].append(row)
                print(json.dumps(row), flush=True)
    out["shared_equals_unshared"] = results[True] == results[False]
    print(json.dumps(dict(shared_equals_unshared=out["shared_equals_unshared"])), flush=True)
    gen = torch.Generator().manual_seed(0)
    st = e._stream()
    for rnd in range(3):
        for n in (8, 128):
            rows = torch.randn(n, V, generator=gen) * 4.0
            for i in range(n):
                rows[i, torch.randperm(V, generator=gen)[:8]] = 4.0 * (4.0 + 2.0 * torch.rand(8, generator=gen))
            lg = rows.float().cuda()
            tg = torch.randint(0, V, (n,), generator=gen).to(torch.int32).cuda()
            lp = torch.empty(n, dtype=torch.float32, device="cuda")
            am = torch.empty(n, dtype=torch.int32, device="cuda")

            def go():
                rc = e.L.aur_score_rows(e.ctx, lg.data_ptr(), n, V, tg.data_ptr(), lp.data_ptr(), am.data_ptr(), st)
                assert rc == 0
            for _ in range(5):
                go()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                go()
            e1.record()
            torch.cuda.synchronize()
            row = dict(rows=n, vocab=V, round=rnd, kernel="score_rows_kernel", us_per_launch=round(e0.elapsed_time(e1) * 1e3 / args.iters, 2))
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

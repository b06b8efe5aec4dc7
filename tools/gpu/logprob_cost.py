#!/usr/bin/env python3
"""What recording the log-probabilities of generated tokens costs (a tool, not a test).

    timeout -k 10 900 python tools/gpu/logprob_cost.py [--out profiles/logprob_cost.json] [--iters 200] [--steps 48]

One process, synthetic weights at AuroraCap-7B shapes (the language model alone):

  * `rows`: microseconds per launch of `token_logprob_rows_kernel` (aur_token_logprob_rows) at top_n 0 / 1 / 8, with
    `score_rows_kernel` (aur_score_rows) on the same rows as the yardstick: rows shaped like a language model's (N(0, 4^2) with 8
    boosted tokens), 8 and 128 rows x 32000, from device events over `--iters` launches, the variants taking turns, three rounds;
  * `decode`: milliseconds per decode step (device events around `--steps` steps replayed from the captured graph, behind a 64-token
    prefill of every slot) on an engine of 8 slots and on one of 128, with the feature off, at top_n 0 and at top_n 8, the arms taking
    turns, three rounds; `share_of_step` is (arm - off) / off inside the same round.

No threshold hangs on the output; DESIGN section 5 quotes this file only.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprob_cost.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=48)
    args = ap.parse_args()
    import torch
    from aurora_amd import synthetic as S
    from aurora_amd._lib import check
    from aurora_amd.engine import AuroraCapEngine

    V = 32000
    lcfg = S.AURORACAP_7B["llm"]
    w = {"llm": S.llm_weights(lcfg)}
    out = dict(device=torch.cuda.get_device_name(0), vocab=V, iters=args.iters, steps=args.steps, rows=[], decode=[])

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n                              # ms per call

    for slots in (8, 128):
        prompt, new = 64, args.steps + 8
        e = AuroraCapEngine({"vit": None, "llm": lcfg}, w, max_frames=1, max_batch=slots, max_ctx=prompt + new + 56, max_new_tokens=new)
        with torch.cuda.stream(e.stream):                           # events and launches on one stream
            st = e._stream()
            if slots == 8:                                           # the kernel alone
                gen = torch.Generator().manual_seed(0)
                for rnd in range(3):
                    for n in (8, 128):
                        rows = torch.randn(n, V, generator=gen) * 4.0
                        for i in range(n):
                            rows[i, torch.randperm(V, generator=gen)[:8]] = 4.0 * (4.0 + 2.0 * torch.rand(8, generator=gen))
                        lg = rows.float().cuda()
                        tg = torch.randint(0, V, (n,), generator=gen).to(torch.int32).cuda()
                        lp = torch.empty(n, dtype=torch.float32, device="cuda")
                        am = torch.empty(n, dtype=torch.int32, device="cuda")
                        tid = torch.empty(n, 8, dtype=torch.int32, device="cuda")
                        tlp = torch.empty(n, 8, dtype=torch.float32, device="cuda")

                        def score():
                            assert e.L.aur_score_rows(e.ctx, lg.data_ptr(), n, V, tg.data_ptr(), lp.data_ptr(), am.data_ptr(), st) == 0

                        def logprob(top):
                            assert e.L.aur_token_logprob_rows(e.ctx, lg.data_ptr(), n, V, tg.data_ptr(), top, lp.data_ptr(), tid.data_ptr(),
                                                              tlp.data_ptr(), st) == 0
                        variants = [("score_rows_kernel", score)] + [(f"token_logprob_rows_kernel top_n={t}", lambda t=t: logprob(t)) for t in (0, 1, 8)]
                        for _, fn in variants:
                            timed(fn, 5)
                        for name, fn in variants:
                            row = dict(rows=n, vocab=V, round=rnd, kernel=name, us_per_launch=round(timed(fn, args.iters) * 1e3, 2))
                            out["rows"].append(row)
                            print(json.dumps(row), flush=True)
            # the decode step
            buf = torch.empty(int(e.L.aur_logprob_bytes(e.ctx, 8)), dtype=torch.uint8, device="cuda")
            emb = torch.randn(prompt, lcfg["hidden_size"], generator=torch.Generator().manual_seed(1)).half().cuda()
            embs = emb.repeat(slots, 1)

            def arm(top):
                """off (None) or recording with top_n; a fresh batch of `slots` sequences behind their first tokens, graph captured"""
                torch.cuda.synchronize()
                check(e.ctx, e.L.aur_logprob_enable(e.ctx, top or 0, None if top is None else buf.data_ptr(), buf.numel(), st), "aur_logprob_enable")
                e.begin_batch(slots, new, None)
                for b0 in range(0, slots, 8):
                    e.prefill_batch(b0, 8, embs[b0 * prompt:(b0 + 8) * prompt].clone(), prompt)
                e.decode(4)                                          # captures the step
                ms = timed(lambda: e.decode(1), args.steps)
                assert e.unfinished() == slots
                return ms
            for rnd in range(3):
                ms = {}
                for top in (None, 0, 8):
                    ms[top] = arm(top)
                for top in (None, 0, 8):
                    row = dict(slots=slots, round=rnd, arm="off" if top is None else f"top_n={top}", ms_per_step=round(ms[top], 4),
                               share_of_step=None if top is None else round((ms[top] - ms[None]) / ms[None], 4))
                    out["decode"].append(row)
                    print(json.dumps(row), flush=True)
            check(e.ctx, e.L.aur_logprob_enable(e.ctx, 0, None, 0, st), "aur_logprob_enable")
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

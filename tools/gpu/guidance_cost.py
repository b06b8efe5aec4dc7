#!/usr/bin/env python3
"""What classifier-free guidance costs a decode step (a tool, not a test).

    timeout -k 10 1100 python tools/gpu/guidance_cost.py [--out profiles/guidance_cost.json] [--steps 32]

One process, synthetic weights at AuroraCap-7B shapes (the language model alone), an engine of 128 slots, batches of 8 and of 128 slots:

  * `launches`: microseconds per guidance_apply_kernel + guidance_restore_kernel + guidance_follow_kernel triple alone
    (aur_microbench "dec_guid": back-to-back launches on the bank's own logits) with every record neutral and with slots / 2 pairs;
  * `decode`: milliseconds per decode step (device events around `--steps` steps replayed from the captured graph, behind a 64-token
    prefill of every slot) with option "guidance" off, on with every slot's record neutral, and on with slots / 2 pairs (leaders in the
    lower half, each with its partner in the upper half), the arms taking turns on fresh batches, three rounds; `share_of_step` is
    (arm - off) / off inside the same round.

A guided request occupies two slots by construction: `pairs` against `off` is the cost of the three launches at equal slot count, not
the cost of a guided caption against an unguided one.  No threshold hangs on the output; DESIGN section 5 quotes this file only.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_cost.json"))
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--scale", type=float, default=1.5)
    args = ap.parse_args()
    import torch
    from aurora_amd import guidance as GD
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine

    lcfg = S.AURORACAP_7B["llm"]
    w = {"llm": S.llm_weights(lcfg)}
    max_slots, prompt = 128, 64
    new = 3 * args.steps + 32
    out = dict(device=torch.cuda.get_device_name(0), vocab=lcfg["vocab_size"], steps=args.steps, iters=args.iters, scale=args.scale,
               prompt=prompt, launches=[], decode=[])
    e = AuroraCapEngine({"vit": None, "llm": lcfg}, w, max_frames=1, max_batch=max_slots, max_ctx=prompt + new + 56, max_new_tokens=new)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n                              # ms per call

    def emit(kind, row):
        out[kind].append(row)
        print(json.dumps(dict(kind=kind, **row)), flush=True)

    with torch.cuda.stream(e.stream):                               # events and launches on one stream
        emb = torch.randn(prompt, lcfg["hidden_size"], generator=torch.Generator().manual_seed(1)).half().cuda()
        embs = emb.repeat(8, 1)

        def fresh(arm, slots):
            """a fresh batch of `slots` slots under off / neutral / pairs: the option (the decode graph is re-captured), the records,
            the prefill - the upper half first, a leader's first pick reads its partner's row - and the step's capture"""
            torch.cuda.synchronize()
            e.set_option("guidance", 0 if arm == "off" else 1)
            e.begin_batch(slots, new, None)
            if arm == "pairs":
                e.slot_guidance(0, GD.records(args.scale, GD.pair_slots(slots // 2, slots), slots))
            for b0 in range(slots - 8, -1, -8):
                e.prefill_batch(b0, 8, embs.clone(), prompt)
            e.decode(4)

        arms = ("off", "neutral", "pairs")
        for slots in (8, 128):
            for rnd in range(3):
                ms = {}
                for arm in arms:
                    fresh(arm, slots)
                    ms[arm] = timed(lambda: e.decode(1), args.steps)
                for arm in arms:
                    emit("decode", dict(slots=slots, pairs=slots // 2 if arm == "pairs" else 0, round=rnd, arm=arm,
                                        ms_per_step=round(ms[arm], 4),
                                        share_of_step=None if arm == "off" else round((ms[arm] - ms["off"]) / ms["off"], 5)))
            for arm in ("neutral", "pairs"):
                fresh(arm, slots)
                emit("launches", dict(slots=slots, pairs=slots // 2 if arm == "pairs" else 0, arm=arm,
                                      us_per_triple=round(e.microbench("dec_guid", args.iters), 2)))
        torch.cuda.synchronize()
        e.set_option("guidance", 0)
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

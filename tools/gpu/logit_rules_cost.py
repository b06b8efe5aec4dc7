#!/usr/bin/env python3
"""What the logit rules (repetition penalty, no-repeat n-gram, min-new-tokens) cost a decode step (a tool, not a test).

    timeout -k 10 1100 python tools/gpu/logit_rules_cost.py [--out profiles/logit_rules_cost.json] [--steps 32] [--history 2047]

One process, synthetic weights at AuroraCap-7B shapes (the language model alone), 128 slots:

  * `decode`: milliseconds per decode step (device events around `--steps` steps replayed from the captured graph, behind a 64-token
    prefill of every slot, so at history lengths 1 ..) with option "logit_rules" off, on with every slot's record neutral, and on with
    every slot's record active (penalty 1.2, no-repeat 3-gram, the EOS held back), the arms taking turns on fresh batches, three
    rounds; `share_of_step` is (arm - off) / off inside the same round;
  * `pair`: microseconds per logit_rules_apply_kernel + logit_rules_restore_kernel pair alone (aur_microbench "dec_rules": back-to-back
    launches on the bank's own logits and history) with neutral and with active records, at the history length the bank is at;
  * `long`: the same engine decoded (option off) until every slot holds `--history` generated tokens, then `pair` again and the step
    in the order off, neutral, active, active, neutral, off - the context grows by a token per step, the mirrored order cancels
    that drift - `--steps` / 4 steps each.

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_rules_cost.json"))
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--history", type=int, default=2047)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import torch
    from aurora_amd import logit_rules as LR
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine

    lcfg = S.AURORACAP_7B["llm"]
    w = {"llm": S.llm_weights(lcfg)}
    slots, prompt, eos = args.slots, 64, 2
    new = args.history + 2 * args.steps + 16
    active = LR.check_logit_rules(dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=new))     # the EOS never comes
    out = dict(device=torch.cuda.get_device_name(0), vocab=lcfg["vocab_size"], slots=slots, steps=args.steps, iters=args.iters,
               active=active, decode=[], pair=[], long=[])
    e = AuroraCapEngine({"vit": None, "llm": lcfg}, w, max_frames=1, max_batch=slots, max_ctx=prompt + new + 56, max_new_tokens=new)

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

    def set_arm(arm):
        """off / neutral / active on the batch in flight: the option (the decode graph is re-captured) and every slot's record"""
        torch.cuda.synchronize()
        e.set_option("logit_rules", 0 if arm == "off" else 1)
        if arm != "off":
            e.slot_logit_rules(0, LR.records(active if arm == "active" else None, slots))

    with torch.cuda.stream(e.stream):                               # events and launches on one stream
        emb = torch.randn(prompt, lcfg["hidden_size"], generator=torch.Generator().manual_seed(1)).half().cuda()
        embs = emb.repeat(slots, 1)

        def fresh(arm):
            set_arm("off")                                           # begin_batch clears the records; the arm's are set behind it
            e.begin_batch(slots, new, eos)
            set_arm(arm)
            for b0 in range(0, slots, 8):
                e.prefill_batch(b0, 8, embs[b0 * prompt:(b0 + 8) * prompt].clone(), prompt)
            e.decode(4)                                              # captures the step

        arms = ("off", "neutral", "active")
        for rnd in range(3):
            ms = {}
            for arm in arms:
                fresh(arm)
                ms[arm] = timed(lambda: e.decode(1), args.steps)
            for arm in arms:
                emit("decode", dict(round=rnd, history="5 .. %d" % (4 + args.steps), arm=arm, ms_per_step=round(ms[arm], 4),
                                    share_of_step=None if arm == "off" else round((ms[arm] - ms["off"]) / ms["off"], 5)))
        for arm in ("neutral", "active"):
            fresh(arm)
            emit("pair", dict(history=5, arm=arm, us_per_pair=round(e.microbench("dec_rules", args.iters), 2)))
        # the long history: the active arm all the way, so that the history holds what the rules leave (no n-gram twice)
        fresh("active")
        done = 5
        while done < args.history:
            n = min(64, args.history - done)
            e.decode(n)
            done += n
        torch.cuda.synchronize()
        assert e.unfinished() == slots
        for arm in ("neutral", "active"):
            set_arm(arm)
            emit("pair", dict(history=done, arm=arm, us_per_pair=round(e.microbench("dec_rules", args.iters), 2)))
        k = max(args.steps // 4, 2)
        ms = {a: [] for a in arms}
        for arm in arms + arms[::-1]:
            set_arm(arm)
            e.decode(2)                                              # captures the step
            ms[arm].append(timed(lambda: e.decode(1), k))
        for arm in arms:
            mean = sum(ms[arm]) / 2
            off = sum(ms["off"]) / 2
            emit("long", dict(history="%d .. %d" % (done, done + 6 * (k + 2)), arm=arm, ms_per_step=round(mean, 4), passes=[round(x, 4) for x in ms[arm]],
                              share_of_step=None if arm == "off" else round((mean - off) / off, 5)))
        assert e.unfinished() == slots
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

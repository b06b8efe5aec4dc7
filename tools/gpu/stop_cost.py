#!/usr/bin/env python3
"""What the stop check (stop ids, stop strings, per-request budgets) costs a decode step (a tool, not a test).

    timeout -k 10 900 python tools/gpu/stop_cost.py [--out profiles/stop_cost.json] [--steps 32]

One process, synthetic weights at AuroraCap-7B shapes (the language model alone), 128 slots, a 32000-entry byte table with tokens of
1 to 8 lower-case letters:

  * `decode`: milliseconds per decode step (device events around `--steps` steps replayed from the captured graph, behind a 64-token
    prefill of every slot) in four arms taking turns on fresh batches, three rounds: option "stop_rules" off; on with every slot's
    record neutral; on with 8 strings of 64 bytes and 8 stop ids on every slot (lower-case strings that never occur: every step gathers
    63 bytes of history and tests every string at every end offset); and, as the yardstick, the option off with the
    `token_logprob_kernel` launch behind the pick (`logprobs=0`).  `share_of_step` is (arm - off) / off inside the same round;
  * `kernel`: microseconds per stop_check_kernel launch alone (aur_microbench "dec_stop": back-to-back launches on the bank's own
    history) with neutral records and with the 8 x 64-byte records.

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stop_cost.json"))
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch
    from aurora_amd import stopping as ST
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine

    lcfg = S.AURORACAP_7B["llm"]
    w = {"llm": S.llm_weights(lcfg)}
    slots, prompt, eos = args.slots, 64, None                  # no EOS: no slot ends inside a timed loop
    new = 3 * args.steps + 16
    rng = np.random.default_rng(7)
    table = ST.table_from_list([bytes(rng.integers(97, 123, int(rng.integers(1, 9))).astype(np.uint8)) for _ in range(lcfg["vocab_size"])])
    heavy = ST.check_stop(dict(strings=[bytes(rng.integers(97, 123, 64).astype(np.uint8)) for _ in range(8)],
                               token_ids=[lcfg["vocab_size"] + i for i in range(8)]), new, table)     # ids no pick can produce
    out = dict(device=torch.cuda.get_device_name(0), vocab=lcfg["vocab_size"], slots=slots, steps=args.steps, iters=args.iters,
               table_bytes=int(len(table[1])), decode=[], kernel=[])
    e = AuroraCapEngine({"vit": None, "llm": lcfg}, w, max_frames=1, max_batch=slots, max_ctx=prompt + new + 56, max_new_tokens=new)
    e.set_stop_vocab(table)

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
        embs = emb.repeat(slots, 1)

        def fresh(arm):
            """off / neutral / strings8x64 / logprobs on a fresh batch: the option (the decode graph is re-captured), then the records"""
            torch.cuda.synchronize()
            e.set_option("stop_rules", 0 if arm in ("off", "logprobs") else 1)
            if arm == "logprobs":
                e._logprobs_on(0)
            else:
                e.logprobs_off()
            e.begin_batch(slots, new, eos)
            if arm == "strings8x64":
                e.slot_stop(0, ST.records([heavy] * slots))
            for b0 in range(0, slots, 8):
                e.prefill_batch(b0, 8, embs[b0 * prompt:(b0 + 8) * prompt].clone(), prompt)
            e.decode(4)                                              # captures the step

        arms = ("off", "neutral", "strings8x64", "logprobs")
        for rnd in range(3):
            ms = {}
            for arm in arms:
                fresh(arm)
                ms[arm] = timed(lambda: e.decode(1), args.steps)
                assert e.unfinished() == slots                      # nothing stopped: every step did the whole check
            for arm in arms:
                emit("decode", dict(round=rnd, history="5 .. %d" % (4 + args.steps), arm=arm, ms_per_step=round(ms[arm], 4),
                                    share_of_step=None if arm == "off" else round((ms[arm] - ms["off"]) / ms["off"], 5)))
        for arm in ("neutral", "strings8x64"):
            fresh(arm)
            e.decode(args.steps)
            emit("kernel", dict(history=5 + args.steps, arm=arm, us_per_launch=round(e.microbench("dec_stop", args.iters), 2)))
            assert e.unfinished() == slots
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

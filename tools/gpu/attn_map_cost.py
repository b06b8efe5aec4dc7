#!/usr/bin/env python3
"""What recording the attention of generated tokens over the prompt costs (a tool, not a test).

    timeout -k 10 900 python tools/gpu/attn_map_cost.py [--out profiles/attn_map_cost.json] [--steps 32] [--prompt 2048]

One process, synthetic weights at AuroraCap-7B shapes (the language model alone): milliseconds per decode step (device events around
`--steps` steps replayed from the captured graph, behind a `--prompt`-token prefill of every slot) on an engine of 8 slots and on one
of 64, with the map off, recorded over all 32 layers and over the last 8, the window the prompt rounded up to 64; the arms take turns,
three rounds; `share_of_step` is (arm - off) / off inside the same round.  The recorder reads K once more per recorded layer and
never V, so a step whose attention is K / V-bound pays about half of its attention time again per recorded layer.

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_map_cost.json"))
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 64])
    args = ap.parse_args()
    import torch
    from aurora_amd import attn_map as AM
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine

    lcfg = S.AURORACAP_7B["llm"]
    layers = lcfg["num_hidden_layers"]
    w = {"llm": S.llm_weights(lcfg)}
    window = AM.window_for(args.prompt)
    out = dict(device=torch.cuda.get_device_name(0), steps=args.steps, prompt=args.prompt, window=window, decode=[])
    arms = [("off", None), (f"all {layers} layers", dict(keys=window)), ("last 8 layers", dict(keys=window, layers=list(range(layers - 8, layers))))]

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n                              # ms per call

    for slots in args.slots:
        prompt, new = args.prompt, args.steps + 8
        e = AuroraCapEngine({"vit": None, "llm": lcfg}, w, max_frames=1, max_batch=slots, max_ctx=prompt + new + 56, max_new_tokens=new)
        with torch.cuda.stream(e.stream):                           # events and launches on one stream
            emb = torch.randn(prompt, lcfg["hidden_size"], generator=torch.Generator().manual_seed(1)).half().cuda()
            group = min(slots, 8)
            embs = emb.repeat(group, 1)

            def arm(am):
                """off (None) or recording; a fresh batch of `slots` sequences behind their first tokens, graph captured"""
                torch.cuda.synchronize()
                if am is None:
                    e.attn_map_off()
                else:
                    e._attn_map_request(am, prompt)
                e.begin_batch(slots, new, None)
                for b0 in range(0, slots, group):
                    e.prefill_batch(b0, group, embs.clone(), prompt)
                e.decode(4)                                          # captures the step
                ms = timed(lambda: e.decode(1), args.steps)
                assert e.unfinished() == slots
                if am is not None:                                   # the record is there: the newest row of every slot holds the prompt's share
                    rows = torch.from_numpy(e.attn_map_state()[:, 4 + args.steps]).double().sum(1)
                    assert float(rows.min()) > 0.0 and float(rows.max()) <= 1.0 + 1e-3, rows
                return ms
            for rnd in range(3):
                ms = {name: arm(am) for name, am in arms}
                for name, _ in arms:
                    row = dict(slots=slots, round=rnd, arm=name, ms_per_step=round(ms[name], 4),
                               share_of_step=None if name == "off" else round((ms[name] - ms["off"]) / ms["off"], 4))
                    out["decode"].append(row)
                    print(json.dumps(row), flush=True)
            e.attn_map_off()
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

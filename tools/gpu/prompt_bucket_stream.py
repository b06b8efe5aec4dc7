#!/usr/bin/env python3
"""What the padded prompt bucket buys a serving loop whose prompts all differ in length (a tool, not a test).

    python tools/gpu/prompt_bucket_stream.py [--out profiles/prompt_bucket_stream.json] [--clips 64] [--passes 3]

synthetic.AURORACAP_7B, 8 frames, token_kept_ratio 0.3, 32 new tokens, 8 slots + 4 spare KV sequences, 64 seeded clips with 64 distinct
prompt lengths inside 128 positions, through `caption_stream` (front ends prefetched beside the decode, one hipGraph replay each).
Two engines in ONE process, `prompt_bucket` 0 and 64: one warm-up pass each, then the variants alternate, `--passes` passes each; the
host clock runs around a pass that ends in a device synchronise.  Per pass the file records the wall seconds, the front-end captures
made during it, the graphs alive after it and whether every clip's ids equal the bucket-0 warm-up's.

There is no threshold on the time.  The conditions (exit status 1 otherwise): all ids equal; bucket 64 captures at most
buckets x spare sequences graphs in its warm-up and none afterwards.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES, RATIO, NEW, SLOTS, SPARE = 8, 0.3, 32, 8, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_bucket_stream.json"))
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine, front_end_bucket_key, splice_rows, tokens_at_layer, tome_r

    cfg = S.AURORACAP_7B
    v = cfg["vit"]
    r = tome_r(v["image_size"], v["image_size"], v["patch_size"], RATIO, v["num_hidden_layers"])
    n_kept = tokens_at_layer((v["image_size"] // v["patch_size"]) ** 2 + 1, r, v["num_hidden_layers"] - 1) - 1
    order = np.random.default_rng(7).permutation(args.clips)            # distinct lengths, in no particular order
    clips = [(S.frames(FRAMES, i), S.prompt_ids(FRAMES, i, n_text=30 + int(order[i]))) for i in range(args.clips)]
    lens = [splice_rows(ids, FRAMES, n_kept)["seq_len"] for _, ids in clips]
    assert len(set(lens)) == args.clips and max(lens) - min(lens) < 128
    buckets = len({front_end_bucket_key(0, 16, FRAMES, 378, 378, r, 0, splice_rows(ids, FRAMES, n_kept), 64)[7:] for _, ids in clips})
    max_ctx = max(lens) + 128 + NEW
    w = {"vit": S.vit_weights(v), "projector": S.projector_weights(v["hidden_size"], cfg["llm"]["hidden_size"]), "llm": S.llm_weights(cfg["llm"])}
    engines, captures = {}, {}
    for pb in (0, 64):
        e = AuroraCapEngine(cfg, w, max_frames=FRAMES, max_batch=SLOTS, max_ctx=max_ctx, max_new_tokens=NEW, spare_slots=SPARE, prompt_bucket=pb)
        captures[pb] = []
        inner = e.graph_capture
        e.graph_capture = (lambda fn, inner=inner, log=captures[pb]: (log.append(1), inner(fn))[1])
        engines[pb] = e
    del w

    def one_pass(pb):
        e = engines[pb]
        torch.cuda.set_stream(e.stream)
        n0 = len(captures[pb])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = dict(e.caption_stream(clips, RATIO, NEW, eos_id=None, slots=SLOTS))
        torch.cuda.synchronize()
        return got, dict(prompt_bucket=pb, wall_s=round(time.perf_counter() - t0, 4), captures=len(captures[pb]) - n0, graphs_alive=len(e._front_graphs))

    ref, first = one_pass(0)
    rows, ok = [dict(first, warm_up=True, ids_equal_bucket0=True)], len(ref) == args.clips and all(len(x) == NEW for x in ref.values())
    for pb, warm in [(64, True)] + [(p, False) for _ in range(args.passes) for p in (0, 64)]:
        got, row = one_pass(pb)
        row.update(warm_up=warm, ids_equal_bucket0=got == ref)
        rows.append(row)
        ok = ok and row["ids_equal_bucket0"]
        if pb == 64:
            ok = ok and (row["captures"] <= buckets * SPARE if warm else row["captures"] == 0)
        print(json.dumps(row), flush=True)
    timed = {pb: [x["wall_s"] for x in rows if x["prompt_bucket"] == pb and not x["warm_up"]] for pb in (0, 64)}
    out = dict(model="synthetic.AURORACAP_7B", frames=FRAMES, token_kept_ratio=RATIO, max_new_tokens=NEW, slots=SLOTS, spare_sequences=SPARE,
               clips=args.clips, prompt_positions=[min(lens), max(lens)], buckets_of_64=buckets, front_graph_cap=engines[0].front_graph_cap,
               device=torch.cuda.get_device_name(0), passes=rows, conditions_hold=bool(ok),
               every_bucket64_pass_faster_than_every_bucket0_pass=bool(timed[0] and timed[64] and max(timed[64]) < min(timed[0])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for e in engines.values():
        e.close()
    print(json.dumps({k: out[k] for k in ("conditions_hold", "every_bucket64_pass_faster_than_every_bucket0_pass")}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

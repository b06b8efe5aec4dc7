#!/usr/bin/env python3
"""What sharing the visual prefix buys a serving loop that asks several questions about every video (a tool, not a test).

    python tools/gpu/shared_prefix_stream.py [--out profiles/shared_prefix_stream.json] [--clips 16] [--prompts 5] [--passes 3]

synthetic.AURORACAP_7B, 8 frames, token_kept_ratio 0.3, 32 new tokens, 8 slots, 16 seeded clips x 5 prompts of different lengths
(the rows up to the last visual token are common to a clip's prompts), siblings adjacent, through `caption_stream` with the front ends
prefetched beside the decode.  Two engines in ONE process: `off` (4 spare KV sequences, no keys) and `on` (one more spare sequence as the
holder, `share_key` = the clip).  One warm-up pass each, then the arms alternate, `--passes` passes each; the host clock runs around a
pass that ends in a device synchronise.  Per pass the file records the wall seconds, the ViT passes (front ends that ran the vision
tower), the rows pushed through the prefill layer stack (strides, as the GEMMs see them) and whether every request's ids equal the
`off` warm-up's.  Then the copy kernel alone on the `on` engine: mean time over 20 launches (device events) and bytes per second (read
once + written ndst times) at 33 pages x 32 layers for 1 and 4 destinations.

There is no threshold on the time.  The conditions (exit status 1 otherwise): all ids equal; the `on` arm runs one ViT pass per clip.
The rule for the adaptor's default (`share_visual_prefix`): on, if every sharing pass beats every non-sharing pass with equal ids.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES, RATIO, NEW, SLOTS, SPARE, BUCKET = 8, 0.3, 32, 8, 4, 64
COPY_PAGES, COPY_ITERS = 33, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix_stream.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--prompts", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine, share_fork, splice_rows, tokens_at_layer, tome_r

    cfg = S.AURORACAP_7B
    v, l = cfg["vit"], cfg["llm"]
    r = tome_r(v["image_size"], v["image_size"], v["patch_size"], RATIO, v["num_hidden_layers"])
    n_kept = tokens_at_layer((v["image_size"] // v["patch_size"]) ** 2 + 1, r, v["num_hidden_layers"] - 1) - 1
    frames = [S.frames(FRAMES, i) for i in range(args.clips)]
    reqs, keys = [], []
    for i in range(args.clips):
        ids0 = S.prompt_ids(FRAMES, i)
        head = ids0[:len(ids0) - ids0[::-1].index(-200)]                 # up to and including the last image marker
        for q in range(args.prompts):                                      # the question: its own tokens, 12 + 9 q of them
            reqs.append((frames[i], head + np.random.default_rng(5000 + q).integers(3, l["vocab_size"], size=12 + 9 * q).tolist()))
            keys.append(i)
    plans = [splice_rows(ids, FRAMES, n_kept) for _, ids in reqs]
    lens = [p["seq_len"] for p in plans]
    forks = [share_fork(plans[k - k % args.prompts], plans[k]) for k in range(len(reqs))]
    assert len(set(lens[:args.prompts])) == args.prompts and all(f > 0 for k, f in enumerate(forks) if k % args.prompts)
    max_ctx = max(lens) + 128 + NEW
    w = {"vit": S.vit_weights(v), "projector": S.projector_weights(v["hidden_size"], l["hidden_size"]), "llm": S.llm_weights(l)}
    engines, vit_passes, rows = {}, {}, {}
    for arm in ("off", "on"):
        e = AuroraCapEngine(cfg, w, max_frames=FRAMES, max_batch=SLOTS, max_ctx=max_ctx, max_new_tokens=NEW, prompt_bucket=BUCKET,
                            spare_slots=SPARE + (arm == "on"), prefix_cache=int(arm == "on"))
        vit_passes[arm], rows[arm] = [], []
        replay, commit, ext = e._front_end_replay, e.prefill_commit, e.extend_commit
        e._front_end_replay = (lambda *a, inner=replay, log=vit_passes[arm]: (log.append(1), inner(*a))[1])
        # rows of a front end, counted where it is committed: the stride of a bucketed prefill, the stride of an extend
        e.prefill_commit = (lambda s, n, q, emb, L, seq_lens=None, inner=commit, log=rows[arm]: (log.append(n * L), inner(s, n, q, emb, L, seq_lens=seq_lens))[1])
        e.extend_commit = (lambda s, n, q, emb, p0, st, nl, inner=ext, log=rows[arm]: (log.append(n * st), inner(s, n, q, emb, p0, st, nl))[1])
        engines[arm] = e
    del w

    def one_pass(arm):
        e = engines[arm]
        torch.cuda.set_stream(e.stream)
        n0, r0 = len(vit_passes[arm]), len(rows[arm])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kw = dict(share_key=lambda k: keys[k]) if arm == "on" else {}
        got = dict(e.caption_stream(reqs, RATIO, NEW, eos_id=None, slots=SLOTS, overlap=True, **kw))
        torch.cuda.synchronize()
        return got, dict(arm=arm, wall_s=round(time.perf_counter() - t0, 4), vit_passes=len(vit_passes[arm]) - n0,
                         rows_prefilled=int(sum(rows[arm][r0:])))

    ref, first = one_pass("off")
    out_rows, ok = [dict(first, warm_up=True, ids_equal=True)], len(ref) == len(reqs) and all(len(x) == NEW for x in ref.values())
    for arm, warm in [("on", True)] + [(a, False) for _ in range(args.passes) for a in ("off", "on")]:
        got, row = one_pass(arm)
        differing = [(k, next((t for t, (x, y) in enumerate(zip(got.get(k, []), ref[k])) if x != y), -1)) for k in sorted(ref) if got.get(k) != ref[k]]
        row.update(warm_up=warm, ids_equal=got == ref, requests_differing=len(differing), first_differences=differing[:8])
        out_rows.append(row)
        ok = ok and row["ids_equal"] and (arm == "off" or row["vit_passes"] == args.clips)
        print(json.dumps(row), flush=True)

    # the copy kernel alone: 33 pages x every layer from sequence 0 into 1 / 4 others (a finished pass left valid pages everywhere)
    e = engines["on"]
    torch.cuda.set_stream(e.stream)
    page_bytes = 2 * l["hidden_size"] * 64 * 2                            # K and V of 64 tokens, fp16
    copy = []
    for ndst in (1, 4):
        e.kv_copy_prefix(0, 1, ndst, COPY_PAGES * 64)                      # warm-up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(torch.cuda.current_stream())
        for _ in range(COPY_ITERS):
            e.kv_copy_prefix(0, 1, ndst, COPY_PAGES * 64)
        t1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / COPY_ITERS
        moved = COPY_PAGES * l["num_hidden_layers"] * page_bytes * (1 + ndst)
        copy.append(dict(ndst=ndst, pages=COPY_PAGES, layers=l["num_hidden_layers"], mean_us=round(us, 1), bytes_moved=moved,
                         bytes_per_s=round(moved / (us * 1e-6), 0)))
        print(json.dumps(copy[-1]), flush=True)

    timed = {a: [x["wall_s"] for x in out_rows if x["arm"] == a and not x["warm_up"]] for a in ("off", "on")}
    out = dict(model="synthetic.AURORACAP_7B", frames=FRAMES, token_kept_ratio=RATIO, max_new_tokens=NEW, slots=SLOTS, spare_sequences=SPARE,
               prompt_bucket=BUCKET, clips=args.clips, prompts_per_clip=args.prompts, prompt_positions=[min(lens), max(lens)],
               fork_positions=sorted(set(f for k, f in enumerate(forks) if k % args.prompts)), device=torch.cuda.get_device_name(0),
               passes=out_rows, ids_equal=bool(all(x["ids_equal"] for x in out_rows)), copy_kernel=copy, conditions_hold=bool(ok),
               every_sharing_pass_faster_than_every_non_sharing_pass=bool(timed["off"] and timed["on"] and max(timed["on"]) < min(timed["off"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for e in engines.values():
        e.close()
    print(json.dumps({k: out[k] for k in ("conditions_hold", "ids_equal", "every_sharing_pass_faster_than_every_non_sharing_pass")}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

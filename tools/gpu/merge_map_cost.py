#!/usr/bin/env python3
"""What the merge map costs the vision tower (a tool, not a test).

    timeout -k 10 900 python tools/gpu/merge_map_cost.py --parent-lib PATH [--out profiles/merge_map_cost.json] [--repeats 5]

8 frames of 378 x 378 at r = 15 (the benchmark's front end: 729 patches -> 264 tokens per frame), synthetic weights at AuroraCap-7B's
ViT shapes.  Three arms:

  * `parent_hw`: aur_vit_encode_hw on the PARENT commit's library (`--parent-lib`: libaurora_hip.so built from the commit before the
    merge map; loaded through AURORA_HIP_SO with the three new symbols taken off the binding's list);
  * `this_hw`:   the same call on this build - it launches the same kernels, so a difference from `parent_hw` beyond the run-to-run
    spread recorded here would be a defect;
  * `this_map`:  aur_vit_encode_map on this build: 2 + (merging layers) more short launches.

A repeat is one fresh child process (one engine, 3 warm-up calls, then `--iters` calls between two device events: milliseconds per
call); the arms take turns, `--repeats` rounds.  The file holds every repeat, and per arm the median and the spread (min, max).
No threshold hangs on the output; DESIGN section 5 quotes this file only.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES, R = 8, 15


def child(arm: str, iters: int) -> int:
    import torch
    from aurora_amd import _lib
    if arm == "parent_hw":                                   # the parent's library does not export what this change adds
        for name in ("aur_vit_encode_map", "aur_tome_map_rows", "aur_unmerge_rows"):
            _lib.SIGNATURES.pop(name, None)
    from aurora_amd import synthetic as S
    from aurora_amd.engine import AuroraCapEngine
    vcfg = S.AURORACAP_7B["vit"]
    e = AuroraCapEngine({"vit": vcfg, "llm": None}, {"vit": S.vit_weights(vcfg)}, max_frames=FRAMES, max_batch=1, max_ctx=128,
                        max_new_tokens=8)
    with torch.cuda.stream(e.stream):                        # events and launches on one stream
        px = S.frames(FRAMES, 0).half().cuda()
        tok = e.vit_encode(px, R)
        outs = tok if arm != "this_map" else e.vit_encode(px, R, merge_map=True)
        run = (lambda: e.vit_encode(px, R, out=outs, merge_map=True)) if arm == "this_map" else (lambda: e.vit_encode(px, R, out=outs))
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
    print(json.dumps(dict(arm=arm, ms_per_call=round(ms, 4), n_kept=int(tok.shape[1]), device=torch.cuda.get_device_name(0))), flush=True)
    e.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_map_cost.json"))
    ap.add_argument("--parent-lib", default=None, help="libaurora_hip.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.iters)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("error: --parent-lib must name the parent commit's libaurora_hip.so")
    if args.repeats < 5:
        sys.exit("error: at least five repeats per arm")
    arms = ("parent_hw", "this_hw", "this_map")
    runs = {a: [] for a in arms}
    device = None
    for rnd in range(args.repeats):
        for arm in arms:
            env = dict(os.environ)
            env.pop("AURORA_HIP_SO", None)
            if arm == "parent_hw":
                env["AURORA_HIP_SO"] = os.path.abspath(args.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm, "--iters", str(args.iters)], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:                            # a failed child ends the measurement: nothing more is started
                sys.stderr.write(r.stderr[-3000:])
                sys.exit(f"error: arm {arm} of round {rnd} ended with status {r.returncode}")
            row = json.loads(r.stdout.strip().split("\n")[-1])
            device = row.pop("device")
            runs[arm].append(row["ms_per_call"])
            print(json.dumps(dict(round=rnd, **row)), flush=True)
    out = dict(device=device, frames=FRAMES, image=378, r=R, iters=args.iters, repeats=args.repeats,
               arms={a: dict(ms_per_call=runs[a], median=round(statistics.median(runs[a]), 4), min=min(runs[a]), max=max(runs[a])) for a in arms})
    m = {a: out["arms"][a]["median"] for a in arms}
    out["this_hw_minus_parent_hw_ms"] = round(m["this_hw"] - m["parent_hw"], 4)
    out["this_map_minus_this_hw_ms"] = round(m["this_map"] - m["this_hw"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "arms"}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the sampled token pick costs beside the greedy one (a tool, not a test).

    timeout -k 10 600 python tools/gpu/sampling_cost.py [--out profiles/sampling_cost.json] [--iters 200] [--rounds 3]

One process, one small language model with the real vocabulary (hidden 512, 2 layers, vocab 32000), engines of 8 and of 128 slots:

  * `pick`: microseconds per launch of the pick kernel alone (aur_microbench "dec_pick": argmax_advance_kernel in mode 0,
    sample_advance_kernel in mode 1) on the logits the engine's own last step left, from device events over `--iters` launches, for
    greedy records, (0.7, 50, 0.9) and (1, 0, 0.9), with the row staged in LDS and re-read from L2 ("sample_stage" 1 / 0); the
    variants alternate, `--rounds` rounds;
  * `rows`: the same pick through aur_sample_rows on rows shaped like a language model's (N(0, 4^2) with 8 boosted tokens) - the tiny
    model's own logits are nearly flat, which is the sampler's easy case for top-k and its hard case for top-p;
  * `step`: the 128-slot decode step (hipGraph replays, device events around 64 steps) in mode 0 and in mode 1 with (0.7, 50, 0.9) on
    every slot.  The tiny model's step is far shorter than the 7B model's, so the pick's share of THIS step is an upper bound in
    absolute microseconds only; DESIGN section 4 relates the microseconds to the real step.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CFG = dict(hidden_size=512, num_attention_heads=4, num_hidden_layers=2, intermediate_size=1024, vocab_size=32000, rms_norm_eps=1e-5,
           rope_theta=1e4, rope_factor=1.0)
SETTINGS = {"greedy": None, "t0.7_k50_p0.9": dict(temperature=0.7, top_k=50, top_p=0.9, seed=1), "t1_k0_p0.9": dict(temperature=1.0, top_k=0, top_p=0.9, seed=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_cost.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from aurora_amd import sampling as S
    from aurora_amd.engine import AuroraCapEngine

    g = torch.Generator().manual_seed(0)
    rn = lambda *s, std=0.05: (torch.randn(*s, generator=g) * std).half().float()
    d, mlp, V = CFG["hidden_size"], CFG["intermediate_size"], CFG["vocab_size"]
    w = {"embed_tokens.weight": rn(V, d, std=1.0), "norm.weight": 1 + rn(d, std=0.1), "lm_head.weight": rn(V, d, std=0.1), "layers": []}
    for _ in range(CFG["num_hidden_layers"]):
        lw = {n + ".weight": rn(d, d) for n in ("q_proj", "k_proj", "v_proj", "o_proj")}
        lw["gate_proj.weight"], lw["up_proj.weight"], lw["down_proj.weight"] = rn(mlp, d), rn(mlp, d), rn(d, mlp)
        lw["input_layernorm.weight"], lw["post_attention_layernorm.weight"] = 1 + rn(d, std=0.1), 1 + rn(d, std=0.1)
        w["layers"].append(lw)
    out = dict(model=CFG, device=None, iters=args.iters, pick=[], rows=[], step=[])
    for slots in (8, 128):
        e = AuroraCapEngine({"vit": None, "llm": CFG}, {"llm": w}, max_frames=1, max_batch=slots, max_ctx=256, max_new_tokens=64)
        out["device"] = torch.cuda.get_device_name(0)
        emb = torch.zeros(slots * 64, d, dtype=torch.float16, device="cuda")
        emb.copy_((torch.randn(slots * 64, d, generator=g) * 0.5).half())

        def fill(samp):
            e.begin_batch(slots, 64, None)
            if samp is not None:
                e.slot_sampling(0, S.records(S.check_sampling(samp), range(slots)))
            e.prefill_batch(0, slots, emb.clone(), 40)
            e.decode(2)

        for rnd in range(args.rounds):
            for mode, stage in ((0, 1), (1, 1), (1, 0)):
                e.set_option("sampling", mode)
                e.set_option("sample_stage", stage)
                for name, samp in SETTINGS.items():
                    if mode == 0 and samp is not None:
                        continue
                    fill(samp)
                    us = e.microbench("dec_pick", args.iters)
                    row = dict(slots=slots, round=rnd, mode=mode, stage_lds=stage, records=name,
                               kernel="sample_advance_kernel" if mode else "argmax_advance_kernel", us_per_launch=round(us, 2))
                    out["pick"].append(row)
                    print(json.dumps(row), flush=True)
        # the pick on language-model-shaped rows, through the kernel-level entry
        rows = torch.randn(slots, V, generator=g) * 4.0
        for i in range(slots):
            rows[i, torch.randperm(V, generator=g)[:8]] = 4.0 * (4.0 + 2.0 * torch.rand(8, generator=g))
        lg = rows.float().cuda()
        tok = torch.empty(slots, dtype=torch.int32, device="cuda")
        kept = torch.empty_like(tok)
        nd = torch.zeros(slots, dtype=torch.int32, device="cuda")
        for rnd in range(args.rounds):
            for stage in (1, 0):
                e.set_option("sample_stage", stage)
                for name, samp in SETTINGS.items():
                    rec = S.records(S.check_sampling(samp) if samp else None, range(slots))
                    prm = torch.from_numpy(rec.view(np.uint8).reshape(slots, -1).copy()).cuda()
                    st = e._stream()

                    def go():
                        rc = e.L.aur_sample_rows(e.ctx, lg.data_ptr(), slots, V, prm.data_ptr(), nd.data_ptr(), tok.data_ptr(), kept.data_ptr(), st)
                        assert rc == 0
                    for _ in range(5):
                        go()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        go()
                    e1.record()
                    torch.cuda.synchronize()
                    row = dict(slots=slots, round=rnd, stage_lds=stage, records=name, kernel="sample_rows_kernel",
                               us_per_launch=round(e0.elapsed_time(e1) * 1e3 / args.iters, 2), median_kept=int(np.median(kept.cpu().numpy())))
                    out["rows"].append(row)
                    print(json.dumps(row), flush=True)
        e.set_option("sample_stage", 1)
        if slots == 128:
            for rnd in range(args.rounds):
                for mode in (0, 1):
                    e.set_option("sampling", mode)
                    fill(SETTINGS["t0.7_k50_p0.9"] if mode else None)
                    e.decode(4)                                      # captures the step's graph
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    e.decode(48)
                    e1.record()
                    torch.cuda.synchronize()
                    row = dict(slots=slots, round=rnd, mode=mode, us_per_step=round(e0.elapsed_time(e1) * 1e3 / 48, 2))
                    out["step"].append(row)
                    print(json.dumps(row), flush=True)
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

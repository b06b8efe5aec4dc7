#!/usr/bin/env python3
"""Regenerates tests/golden/g20_merge_source.npz: what the reference's own merge module says about which input rows end in which
output row, over chains of ToMe steps.

    python tests/golden/make_golden_merge_source.py        (needs the reference tree, CPU only, a few seconds)

The reference's tome.py is imported the way make_golden.py imports it, and its index tensors are recovered with make_golden's
`tome_indices`.  Per layer of a case the script runs `bipartite_soft_matching(metric, r, class_token=True)` on a seeded randn metric
(generated here, not stored: the code under test consumes indices, not metrics), then `merge_source` (tome.py:222-232) and
`merge_wavg` (tome.py:207-219) through the returned `merge`, and keeps the `unmerge` closure (tome.py:83-98).

Stored per case `c` (DATA ONLY):
  c_meta              int32 [frames, t0, r, layers, d]
  c_L<l>_unm/src/dst  int32 [frames, .] of layer l (empty where the layer does not merge)
  c_group             int32 [frames, t0]: the reference's final `source` [frames, t_final, t0] reduced to the row that holds each column's
                      single 1 (asserted: every column holds exactly one 1, everything else is 0)
  c_size              fp32 [frames, t_final]: the final size of merge_wavg
  c_x                 fp16 [frames, t_final, 8]: the final x of merge_wavg, rounded to fp16
  c_unmerged          fp16 [frames, t0, 8]: the `unmerge` closures applied to c_x from the last layer back to the first
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

D = 8

# name -> (frames, t0, r, layers, metric channels, seed, tie)
CASES = {
    "path15": (2, 730, 15, 31, 16, 2001, False),          # the benchmark shape: 730 -> 265 rows
    "path22": (2, 730, 22, 31, 16, 2002, False),
    "clamp": (1, 10, 5, 5, 8, 2003, False),               # 10 -> 6 -> 4 -> 3 -> 2 -> 2: the (t - 1) // 2 clamp, then a layer that does not merge
    "tiny": (2, 17, 2, 4, 8, 2004, False),                # the tiny encoder of the ViT tests
    "mid": (3, 82, 6, 7, 12, 2005, False),
    "tie": (1, 9, 2, 2, 4, 2006, True),                   # all non-class metric rows identical
    "nonsquare": (2, 1 + 20 * 31, 13, 6, 16, 2007, False),
}


def run_case(tome, frames, t0, r, layers, c, seed, tie):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(frames, t0, D, generator=g)
    size, source = None, None
    out, unmerges, t = {}, [], t0
    for l in range(layers):
        metric = torch.randn(frames, t, c, generator=g)
        if tie:
            metric[:, 1:] = metric[:, 1:2]
        idx, merge = mg.tome_indices(tome, metric, r)
        if idx is None:
            empty = np.zeros((frames, 0), np.int32)
            out[f"L{l}_unm"], out[f"L{l}_src"], out[f"L{l}_dst"] = empty, empty, empty
            # the reference's do_nothing still goes through merge_source / merge_wavg
            source = tome.merge_source(merge, x, source)
            x, size = tome.merge_wavg(merge, x, size)
            continue
        # the helper hands back `merge` only; `unmerge` comes from a second, identical call (same metric: asserted same indices)
        merge2, unmerge = tome.bipartite_soft_matching(metric, r, class_token=True)
        cells = dict(zip(merge2.__code__.co_freevars, [c_.cell_contents for c_ in merge2.__closure__]))
        for k in ("unm_idx", "src_idx", "dst_idx"):
            assert torch.equal(idx[k], cells[k][..., 0])
        out[f"L{l}_unm"] = idx["unm_idx"].numpy().astype(np.int32)
        out[f"L{l}_src"] = idx["src_idx"].numpy().astype(np.int32)
        out[f"L{l}_dst"] = idx["dst_idx"].numpy().astype(np.int32)
        source = tome.merge_source(merge, x, source)
        x, size = tome.merge_wavg(merge, x, size)
        unmerges.append(unmerge)
        t -= idx["r"]
    src = source.numpy()
    assert src.shape == (frames, t, t0)
    assert np.all((src == 0) | (src == 1)) and np.all(src.sum(axis=1) == 1), "a column of `source` does not hold exactly one 1"
    out["group"] = src.argmax(axis=1).astype(np.int32)
    out["size"] = size[..., 0].numpy().astype(np.float32)
    xf = x.half()
    y = xf.float()
    for un in reversed(unmerges):
        y = un(y)
    assert y.shape == (frames, t0, D)
    out["x"] = xf.numpy()
    out["unmerged"] = y.half().numpy()
    assert np.array_equal(out["unmerged"].astype(np.float32), y.numpy())
    out["meta"] = np.array([frames, t0, r, layers, D], np.int32)
    return out, t


def main():
    tome = mg._load("xtuner.model.tome", os.path.join(mg.XT, "model/tome.py"))
    arrs = {}
    for name, spec in CASES.items():
        out, t = run_case(tome, *spec)
        print(f"{name}: frames {spec[0]}  t0 {spec[1]}  r {spec[2]}  layers {spec[3]}  ->  {t} rows")
        for k, v in out.items():
            arrs[f"{name}_{k}"] = v
    arrs["cases"] = np.array(list(CASES))
    mg.save("g20_merge_source.npz", dict(torch=torch.__version__), **arrs)


if __name__ == "__main__":
    main()

"""Regenerates tests/golden/g18_sampling.npz: what transformers' own warpers keep on the 2560 seeded rows of tests/sampling_cases.py,
and how far the float32 pipeline's cumulative distribution lies from the float64 one - the figure the GPU test's epsilon comes from.

    python tests/golden/make_golden_sampling.py

Stored: the seeds, sigmas and settings of every row, the size of the kept set under TemperatureLogitsWarper -> TopKLogitsWarper ->
TopPLogitsWarper in float64 and in float32, and per row max |CDF32 - CDF64| over the kept tokens in index order (softmax and cumsum in
the pipeline's own dtype); `f32_cdf_dev` is the largest of them.  The rows themselves are not stored (regenerated from the seeds)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.sampling_cases import golden_cases  # noqa: E402


def hf_kept(row: torch.Tensor, T: float, k: int, p: float) -> torch.Tensor:
    """processed scores [vocab] (-inf where removed) in row's dtype, through transformers' warpers in their generate() order"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = row[None]
    if T != 1.0:
        s = TemperatureLogitsWarper(float(T))(None, s)
    if k > 0:
        s = TopKLogitsWarper(top_k=int(k))(None, s)
    if p < 1.0:
        s = TopPLogitsWarper(top_p=float(p))(None, s)
    return s[0]


def main():
    import transformers
    cases = golden_cases()
    n = len(cases)
    kept64, kept32, dev = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    from tests.sampling_cases import make_row
    for i, seed, sigma, (T, k, p) in cases:
        row = torch.from_numpy(make_row(seed, sigma))
        s64, s32 = hf_kept(row.double(), T, k, p), hf_kept(row.float(), T, k, p)
        m64, m32 = torch.isfinite(s64), torch.isfinite(s32)
        kept64[i], kept32[i] = int(m64.sum()), int(m32.sum())
        if bool((m64 == m32).all()):
            c64 = torch.cumsum(torch.softmax(s64, -1), -1)[m64]
            c32 = torch.cumsum(torch.softmax(s32, -1), -1)[m32].double()
            dev[i] = float((c64 - c32).abs().max())
        else:
            dev[i] = np.nan
        if i % 256 == 0:
            print(i, seed, sigma, (T, k, p), kept64[i], kept32[i], dev[i], flush=True)
    out = os.path.join(ROOT, "tests", "golden", "g18_sampling.npz")
    np.savez_compressed(out, seeds=np.asarray([c[1] for c in cases], np.int64), sigmas=np.asarray([c[2] for c in cases], np.float64),
                        settings=np.asarray([c[3] for c in cases], np.float64), kept_f64=kept64, kept_f32=kept32, cdf_dev=dev,
                        f32_cdf_dev=np.float64(np.nanmax(dev)), sets_differ=np.int32(np.isnan(dev).sum()),
                        transformers_version=np.asarray(transformers.__version__))
    print("wrote", out, "f32_cdf_dev", float(np.nanmax(dev)), "rows whose f32 / f64 sets differ", int(np.isnan(dev).sum()),
          "median kept", [int(np.median(kept64[j:j + 256])) for j in range(0, n, 256)])


if __name__ == "__main__":
    main()

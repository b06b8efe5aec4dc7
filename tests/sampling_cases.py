"""The seeded logits rows and settings shared by the sampling tests (CPU and GPU) and tests/golden/make_golden_sampling.py.
Rows are regenerated from their seeds by a CPU torch.Generator: 2560 x 32000 floats are not a fixture."""
import numpy as np
import torch

VOCAB = 32000
SETTINGS = [(0.7, 50, 0.9), (1.0, 0, 0.9), (0.2, 0, 0.95), (1.0, 50, 1.0), (1.5, 0, 0.5)]      # (temperature, top_k, top_p)
SIGMAS = (2.0, 4.0)
ROWS_PER_CASE = 256                       # x 5 settings x 2 sigmas = 2560 rows
GOLDEN_SEED0 = 18000


def make_row(seed: int, sigma: float, vocab: int = VOCAB) -> np.ndarray:
    """fp32 [vocab]: N(0, sigma^2) with 8 boosted tokens (4 .. 6 sigma above zero, at seeded places) - the shape of a language
    model's row: a few candidates above a wide tail."""
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(vocab, generator=g) * sigma
    idx = torch.randperm(vocab, generator=g)[:8]
    row[idx] = sigma * (4.0 + 2.0 * torch.rand(8, generator=g))
    return row.float().numpy()


def golden_cases():
    """[(case index, seed, sigma, (T, k, p))] of the 2560 rows, in the order g18_sampling.npz stores its per-row figures."""
    out, i = [], 0
    for si, setting in enumerate(SETTINGS):
        for gi, sigma in enumerate(SIGMAS):
            for r in range(ROWS_PER_CASE):
                out.append((i, GOLDEN_SEED0 + (si * len(SIGMAS) + gi) * ROWS_PER_CASE + r, sigma, setting))
                i += 1
    return out


def chi2_stat(counts: np.ndarray, probs: np.ndarray, n: int):
    """Pearson statistic of observed `counts` against `probs` over n draws, cells with expectation < 5 pooled into one;
    returns (statistic, degrees of freedom)."""
    exp = probs * n
    big = exp >= 5.0
    o, e = list(counts[big].astype(np.float64)), list(exp[big])
    if (~big).any():
        o.append(float(counts[~big].sum()))
        e.append(float(exp[~big].sum()))
    o, e = np.asarray(o), np.asarray(e)
    ok = e > 0
    assert o[~ok].sum() == 0, "a draw landed where the distribution has no mass"
    return float(((o[ok] - e[ok]) ** 2 / e[ok]).sum()), int(ok.sum()) - 1

"""Shared inputs of the guided decode tests (tests/test_gpu_guidance.py) and the margin rule they hold the ids to.  The seeds were
chosen on the CPU, from the fp32 oracle alone (`oracle_guided_greedy` below): free-running guided greedy decodes whose top-2 margin of
the guided row exceeds twice the guided-row bound at all but at most an eighth of the positions - half of what the tests allow - at every
scale the tests use, with and without the logit rules."""
import numpy as np
import torch

from aurora_amd import guidance as GD
from aurora_amd import logit_rules as LR
from oracle import aurora_oracle as O
from tests import guidance_ref as R
from tests.parity_bounds import LOGIT_TOL

# per config: (seed, prompt rows, negative rows, new tokens) - prompts of 40 .. 130 rows, negatives of 8 .. 40 rows: each pair sits on
# pages of different lengths
PAIRS = {
    "hd32": [(39, 40, 8, 24), (31, 97, 33, 16), (53, 130, 40, 12), (56, 65, 17, 20)],
    "hd128": [(42, 43, 9, 24), (31, 101, 40, 16), (30, 128, 25, 12), (38, 70, 31, 20)],
}


def pair_embeds(cfg, seed, Lc, Ln):
    """a prompt's and its negative's embeddings (fp16-representable): the negative is a different, shorter sequence"""
    gen = torch.Generator().manual_seed(1000 + seed)
    c = torch.randn(Lc, cfg["hidden_size"], generator=gen).half().float()
    u = torch.randn(Ln, cfg["hidden_size"], generator=gen).half().float()
    return c, u


def _rows(emb, ids, w, cfg):
    full = torch.cat([emb, w["embed_tokens.weight"][torch.tensor(ids[:-1], dtype=torch.long)]], 0) if len(ids) > 1 else emb
    h, _ = O.llama_forward(full, w, cfg, None, 0)
    return torch.nn.functional.linear(h[emb.shape[0] - 1:], w["lm_head.weight"]).numpy()


def guided_row_bound(rc, ru, g, scale):
    """The guided-row bound: the logit bound of the comparison against the oracle (LOGIT_TOL, relative to the largest |logit|) times
    |g| + |g - 1| - out = g lc + (1 - g) lu -, plus the kernel's own bound against the definition (tests/guidance_ref.py)"""
    return LOGIT_TOL * scale * (abs(g) + abs(g - 1)) + R.bound(rc, ru, g)


def guided_margin_check(ids, c, u, w, cfg, g, rules=None, tag=None, strict=True):
    """Teacher-forced with `ids`: the oracle's two rows at every position, combined by `guidance.apply` (then `logit_rules.apply` over
    the ids so far).  Wherever the top-2 margin of that row exceeds twice the guided-row bound, ids[i] must be its argmax.  Returns
    the number of positions the margin rule skipped."""
    rc, ru = _rows(c, ids, w, cfg), _rows(u, ids, w, cfg)
    scale = float(max(np.abs(rc).max(), np.abs(ru).max()))
    skipped = 0
    for i, t in enumerate(ids):
        row = GD.apply(rc[i], ru[i], g)
        if rules is not None:
            row = LR.apply(row.astype(np.float32), ids[:i], rules, None).astype(np.float64)
        top = np.sort(row)[-2:]
        if top[1] - top[0] > 2 * guided_row_bound(rc[i], ru[i], g, scale):
            if strict:
                assert int(np.argmax(row)) == t, (tag, i, t, int(np.argmax(row)), float(top[1] - top[0]))
            elif int(np.argmax(row)) != t:
                return None
        else:
            skipped += 1
    return skipped


def oracle_guided_greedy(c, u, w, cfg, g, n_new, rules=None):
    """The oracle alone, free running: the guided greedy ids (CPU; how the seeds above were chosen)"""
    ids = []
    for _ in range(n_new):
        rc = _rows(c, ids + [0], w, cfg)[-1]
        ru = _rows(u, ids + [0], w, cfg)[-1]
        row = GD.apply(rc, ru, g)
        if rules is not None:
            row = LR.apply(row.astype(np.float32), ids, rules, None)
        ids.append(int(np.argmax(row)))
    return ids

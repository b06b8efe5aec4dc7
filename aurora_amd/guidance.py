"""Classifier-free guidance ahead of the token pick as this package defines it, in numpy / float64.  No GPU, no torch.

    out = apply(c, u, g)

is what `guidance_apply_kernel` leaves in the leader's logits row before the pick - greedy or sampled - up to the fp32 rounding that
tests/guidance_ref.py bounds.  c is the row conditioned on the prompt (the leader slot's), u the row conditioned on the negative prompt
(its partner's), both over the same vocabulary, g the scale - finite, positive and not 1:

    lc_i = (c_i - max c) - log sum_j exp(c_j - max c)
    lu_i likewise from u
    out_i = g * (lc_i - lu_i) + lu_i

This is transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__, which is the FIRST processor of
GenerationMixin._get_logits_processor: guidance, then the logit rules (`aurora_amd.logit_rules`), then temperature / top-k / top-p or the
argmax.  `out` replaces the leader's row for the pick alone: behind it the row is the model's again, so log-probabilities (`logprobs=`)
stay those of the model's unmodified conditional distribution.  The token picked from the guided row is appended to BOTH sequences, and
both stop together: on the EOS, on a full output row or on the leader's stop record.

g == 1 is no request (transformers does not instantiate the processor, and the ids are exactly the unguided ones).  Rows are assumed
finite - the model's rows are, since the rules that write -inf come after guidance.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

# aur_guidance (include/aurora_hip.h), field for field; the all-zero record is neutral
RECORD = np.dtype([("scale", "<f4"), ("partner", "<i4")])
KEYS = ("scale", "negative", "negative_ids")


def log_softmax(row, dtype=np.float64) -> np.ndarray:
    """(l - max l) - log sum exp(l - max l) of one row"""
    l = np.asarray(row, dtype=dtype)
    z = l - l.max()
    return z - np.log(np.exp(z).sum(dtype=dtype))


def apply(c, u, g: float, dtype=np.float64) -> np.ndarray:
    """The guided row of the conditional row c and the unconditional row u at scale g."""
    lc, lu = log_softmax(c, dtype), log_softmax(u, dtype)
    if lc.shape != lu.shape or lc.ndim != 1:
        raise ValueError(f"rows of shapes {lc.shape} and {lu.shape}")
    return dtype(g) * (lc - lu) + lu


def check_scale(scale) -> Optional[float]:
    """A `guidance_scale`: None and 1 are no request (None comes back); otherwise the finite, positive value the kernel sees (fp32)."""
    if scale is None:
        return None
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)):
        raise ValueError(f"guidance scale must be a number, got {scale!r}")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"guidance scale must be finite and positive (1 = off), got {scale!r}")
    with np.errstate(over="ignore"):
        g = float(np.float32(scale))
    if not (np.isfinite(g) and g > 0):
        raise ValueError(f"guidance scale {scale!r} is not a finite positive float32")
    return None if g == 1.0 else g


def check_guidance(guidance: Optional[dict]) -> Optional[dict]:
    """Validated copy of a `guidance=` argument: dict(scale=g, negative=... | negative_ids=...).  Returns None for None and for a scale
    of None or 1: such a request takes the path of one that never asked.  ValueError for a scale that is not finite and positive."""
    if guidance is None:
        return None
    if not isinstance(guidance, dict):
        raise ValueError(f"guidance must be a dict(scale=..., ...) or None, got {type(guidance).__name__}")
    unknown = set(guidance) - set(KEYS)
    if unknown:
        raise ValueError(f"guidance: unknown keys {sorted(unknown)}")
    g = check_scale(guidance.get("scale"))
    if g is None:
        return None
    out = dict(guidance)
    out["scale"] = g
    return out


def pair_slots(n_requests: int, max_batch: int) -> List[Tuple[int, int]]:
    """(leader, partner) slots of n guided requests: leaders in [0, n), partners in [n, 2n).  A guided request costs two slots."""
    n = int(n_requests)
    if n < 1:
        raise ValueError(f"{n} guided requests")
    if 2 * n > max_batch:
        raise ValueError(f"{n} guided requests need {2 * n} slots; the engine was built with max_batch={max_batch}")
    return [(i, n + i) for i in range(n)]


def records(scale: Optional[float], pairs, count: int) -> np.ndarray:
    """`count` aur_guidance records: the leader of every (leader, partner) pair names its partner at `scale`; every other slot - the
    partners among them - is neutral."""
    out = np.zeros(count, RECORD)
    if scale is not None:
        for lead, part in pairs:
            if not (0 <= lead < count and 0 <= part < count and lead != part):
                raise ValueError(f"pair ({lead}, {part}) outside {count} slots")
            out[lead] = (scale, part)
    return out

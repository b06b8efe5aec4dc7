"""Logit rules ahead of the token pick as this package defines them, restated in numpy / float32.  No GPU, no torch.

    processed = apply(row, history, rules, eos_id)

is what `logit_rules_apply_kernel` leaves in one fp32 logits row before the pick - greedy or sampled - bit for bit.  The definition is
transformers' RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor
(prompt_length_to_skip=0) on the raw row.

The history `h` is the tokens GENERATED so far for that request (`out_ids[b][0:out_len[b]]`), NOT the prompt: the reference calls
`generate(inputs_embeds=...)`, and transformers then starts `input_ids` empty, so its processors never see the prompt either.  With
n = len(h):

  * repetition_penalty p > 0 (1.0 = off): for every DISTINCT token t of h, once however often it occurs,
    l[t] = l[t] * p if l[t] < 0 else l[t] / p, in fp32 with a correctly rounded divide;
  * no_repeat_ngram_size g >= 0 (0 = off): if n + 1 >= g, then for every i in [0, n - g + 1) with h[i : i+g-1] == h[n-g+1 : n],
    l[h[i+g-1]] = -inf; g = 1 bans every generated token;
  * min_new_tokens m >= 0: while n < m, l[eos] = -inf; skipped when there is no EOS (eos_id None or < 0).

A ban wins over a penalty on the same index (-inf * p = -inf / p = -inf), so the result does not depend on the order of the rules.
Log-probabilities (`logprobs=`) stay those of the model's unmodified row.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

# aur_logit_rules (include/aurora_hip.h), field for field
RECORD = np.dtype([("repetition_penalty", "<f4"), ("no_repeat_ngram", "<i4"), ("min_new_tokens", "<i4"), ("reserved", "<i4")])
KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens")
NEUTRAL = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)


def banned_by_ngram(history: Sequence[int], g: int) -> list:
    """The tokens that would complete a g-gram the history already holds (NoRepeatNGramLogitsProcessor), in history order."""
    h = [int(t) for t in history]
    n = len(h)
    if g <= 0 or n + 1 < g:
        return []
    tail = h[n - g + 1:n]
    return [h[i + g - 1] for i in range(n - g + 1) if h[i:i + g - 1] == tail]


def apply(row, history: Sequence[int], rules: Optional[dict], eos_id: Optional[int]) -> np.ndarray:
    """The processed copy of one fp32 logits row.  rules: dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0), any
    key optional, or None (nothing).  Tokens outside [0, vocab) in the history are ignored, as the kernel ignores them."""
    l = np.array(row, dtype=np.float32, copy=True)
    if rules is None:
        return l
    V = l.shape[0]
    p = np.float32(rules.get("repetition_penalty", 1.0))
    g, m = int(rules.get("no_repeat_ngram_size", 0)), int(rules.get("min_new_tokens", 0))
    if not p > 0:                       # the kernel's clamp; check_logit_rules rejects such values before they get here
        p = np.float32(1.0)
    h = [int(t) for t in history]
    n = len(h)
    if p != 1.0:
        t = np.unique(np.asarray([x for x in h if 0 <= x < V], np.int64))
        o = l[t]
        with np.errstate(all="ignore"):
            l[t] = np.where(o < 0, o * p, o / p).astype(np.float32)
    for t in banned_by_ngram(h, max(g, 0)):
        if 0 <= t < V:
            l[t] = -np.inf
    if eos_id is not None and 0 <= int(eos_id) < V and n < m:
        l[int(eos_id)] = -np.inf
    return l


def check_logit_rules(rules: Optional[dict]) -> Optional[dict]:
    """Validated copy of a `logit_rules=` argument: dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0), any key
    optional (a value of None = the neutral one).  Returns None for None and for an all-neutral dict: such a request takes the path of
    one that never asked.  transformers raises ValueError for the same values (a penalty that is not a strictly positive float, a
    negative size or length)."""
    if rules is None:
        return None
    unknown = set(rules) - set(KEYS)
    if unknown:
        raise ValueError(f"logit_rules: unknown keys {sorted(unknown)}")
    p, g, m = (NEUTRAL[k] if rules.get(k) is None else rules[k] for k in KEYS)
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not (p > 0 and np.isfinite(p)):
        raise ValueError(f"repetition_penalty must be a strictly positive number (1.0 = off), got {p!r}")
    for name, v in (("no_repeat_ngram_size", g), ("min_new_tokens", m)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 31:
            raise ValueError(f"{name} must be an integer >= 0 (0 = off), got {v!r}")
    p = float(np.float32(p))            # the value the kernel sees
    if p == 1.0 and g == 0 and m == 0:
        return None
    return dict(repetition_penalty=p, no_repeat_ngram_size=int(g), min_new_tokens=int(m))


def records(rules: Optional[dict], count: int) -> np.ndarray:
    """`count` aur_logit_rules records (numpy, RECORD) of one validated `logit_rules` dict; None = neutral records."""
    out = np.zeros(count, RECORD)
    out["repetition_penalty"] = 1.0
    if rules is not None:
        out["repetition_penalty"] = rules.get("repetition_penalty", 1.0)
        out["no_repeat_ngram"] = rules.get("no_repeat_ngram_size", 0)
        out["min_new_tokens"] = rules.get("min_new_tokens", 0)
    return out

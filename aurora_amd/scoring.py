"""Scoring a given continuation as this package defines it, restated in numpy / float64.  No GPU, no torch.

    lp, a = score_row(logits_row, target)

is what `score_rows_kernel` computes from an fp32 logits row - up to the kernel's fp32 `exp`, `log` and additions, which the GPU
tests bound:

  * a  = the first index of the row's maximum (torch.argmax's rule, which the reference adaptor uses: lmms_eval/models/auroracap.py:290);
  * lp = l[t] - l[a] - log(sum_i exp(l[i] - l[a])): the log-softmax at the target, with the maximum subtracted first.

A continuation c[0 .. n) behind a context of Lc positions is scored from the hidden states of positions Lc - 1 .. Lc + n - 2 of the
sequence `context + c[:-1]`: position Lc - 1 + j predicts c[j].  `score_continuation` takes those n logits rows and returns

    sum_logprob = sum_j lp_j   (float64, in token order)        is_greedy = all(a_j == c[j])

which is the (log-likelihood, is_greedy) pair of lmms_eval/api/model.py:30-53.  An empty continuation is (0.0, True).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def score_row(logits: np.ndarray, target: int) -> Tuple[float, int]:
    """(log-probability of `target`, first argmax) of one logits row, in float64."""
    l = np.asarray(logits, dtype=np.float64).reshape(-1)
    t = int(target)
    if not 0 <= t < l.shape[0]:
        raise ValueError(f"target {t} outside [0, {l.shape[0]})")
    a = int(np.argmax(l))                          # numpy, like torch: the first maximum
    lp = l[t] - l[a] - np.log(np.sum(np.exp(l - l[a])))
    return float(lp), a


def score_rows(logits: np.ndarray, targets: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """`score_row` over the rows of a [rows, vocab] array -> (float64 [rows], int32 [rows]).  A target outside [0, vocab) marks an
    unused entry, as in the kernel: (0.0, -1)."""
    lg = np.asarray(logits)
    lp, am = np.zeros(len(targets), np.float64), np.full(len(targets), -1, np.int32)
    for j, t in enumerate(targets):
        if 0 <= int(t) < lg.shape[1]:
            lp[j], am[j] = score_row(lg[j], int(t))
    return lp, am


# ---------------------------------------------------------------------------------------- log-probabilities of GENERATED tokens
# The token a generation step picked from an fp32 logits row l - by the greedy or by the sampled pick - has the log-probability
# `score_row` gives it under that row: the model's UNMODIFIED distribution (temperature, top-k and top-p do not enter; the rule of the
# reference tree's serving engine, sglang/srt/layers/logits_processor.py:187-218), so greedy captions, sampled captions and
# `loglikelihood` speak of one quantity.  Its top-n alternatives, 0 <= n <= MAX_TOP_LOGPROBS, are the first n entries of the row in the
# order (value descending, index ascending), each with its own lp: rank 0 is `score_row`'s first argmax with lp = -log S, ties go to
# the lower index (the all-equal row gives ids 0 .. n-1), ranks at or beyond the vocabulary are (-1, 0.0).  A token outside [0, vocab)
# marks an unused entry, as in `score_rows`: lp = 0, every rank (-1, 0.0).  A row without a maximum (all NaN) follows `score_row`:
# rank 0 is token 0, and nothing is behind it.
MAX_TOP_LOGPROBS = 8


def check_logprobs(logprobs):
    """The `logprobs=` argument of the generation calls: None (off) or an int in [0, MAX_TOP_LOGPROBS] -> None or that int."""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)):
        raise ValueError(f"logprobs must be None or an int in [0, {MAX_TOP_LOGPROBS}], got {logprobs!r}")
    if not 0 <= int(logprobs) <= MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs={int(logprobs)} outside [0, {MAX_TOP_LOGPROBS}]")
    return int(logprobs)


def token_logprobs(logits: np.ndarray, token: int, top_n: int = 0) -> Tuple[float, np.ndarray, np.ndarray]:
    """(lp of `token`, top ids int32 [top_n], their lp float64 [top_n]) of one logits row, in float64."""
    top_n = check_logprobs(top_n)
    l = np.asarray(logits, dtype=np.float64).reshape(-1)
    ids, lps = np.full(top_n, -1, np.int32), np.zeros(top_n, np.float64)
    t = int(token)
    if not 0 <= t < l.shape[0]:
        return 0.0, ids, lps
    lp, a = score_row(l, t)
    log_s = np.log(np.sum(np.exp(l - l[a])))
    order = np.argsort(-l, kind="stable")                  # value descending, index ascending among equals; NaN last
    order = order[~np.isnan(l[order])]
    if order.shape[0] == 0:
        order = np.array([a])                              # no maximum: score_row's token alone
    k = min(top_n, order.shape[0])
    ids[:k] = order[:k]
    lps[:k] = (l[order[:k]] - l[a]) - log_s
    return lp, ids, lps


def token_logprob_rows(logits: np.ndarray, tokens: Sequence[int], top_n: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`token_logprobs` over the rows of a [rows, vocab] array -> (float64 [rows], int32 [rows, top_n], float64 [rows, top_n])."""
    lg = np.asarray(logits)
    n = len(tokens)
    lp, ids, lps = np.zeros(n, np.float64), np.full((n, top_n), -1, np.int32), np.zeros((n, top_n), np.float64)
    for j, t in enumerate(tokens):
        lp[j], ids[j], lps[j] = token_logprobs(lg[j], int(t), top_n)
    return lp, ids, lps


def score_continuation(logits: np.ndarray, continuation: Sequence[int]) -> Tuple[float, bool, List[float]]:
    """logits [n, vocab]: the rows that predict continuation[0 .. n) -> (sum_logprob, is_greedy, per-token log-probabilities)."""
    cont = [int(t) for t in continuation]
    if not cont:
        return 0.0, True, []
    lg = np.asarray(logits)
    if lg.ndim != 2 or lg.shape[0] != len(cont):
        raise ValueError(f"{lg.shape} logits for a continuation of {len(cont)} tokens")
    lps, greedy = [], True
    for j, t in enumerate(cont):
        lp, a = score_row(lg[j], t)
        lps.append(lp)
        greedy = greedy and a == t
    return combine(lps, greedy)


def combine(token_logprobs: Sequence[float], greedy: bool) -> Tuple[float, bool, List[float]]:
    """The per-token values of one continuation -> (their float64 sum in token order, is_greedy, the values)."""
    total = 0.0
    for lp in token_logprobs:
        total += float(lp)
    return total, bool(greedy), [float(x) for x in token_logprobs]

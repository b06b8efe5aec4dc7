"""Seeded sampling as this package defines it, restated in numpy / float64.  No GPU, no torch.

    token, kept, (idx, lo, hi) = reference_pick(logits, T, k, p, seed, stream, n)

is the token `sample_advance_kernel` draws for token index `n` of request `stream` under `seed` from the fp32 logits row - up to the
kernel's fp32 `exp` and its 2^-40 fixed-point weights, which the GPU tests bound.  The order of operations is transformers'
(TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial), restated with value thresholds so that
it needs no sort and no tie-break by position:

  * s_i = logit_i / T, e_i = exp(s_i - max s);
  * top-k (k > 0, else off; k >= vocab keeps everything): tau_k = the k-th largest s, keep s_i >= tau_k (ties at the threshold stay);
  * top-p (0 < p < 1, else off) on what top-k kept, mass Z_k: keep s_i iff the kept values STRICTLY greater than s_i weigh less than
    p * Z_k - equal values stand or fall together; the maximum is always kept;
  * u = (x0 >> 8) * 2^-24, x0 = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (n, stream, 0, 0);
    token = the smallest kept index whose inclusive weight sum exceeds u * Z_K; if rounding leaves none, the largest kept index;
  * T == 0: greedy, the first maximum.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF

# aur_sampling (include/aurora_hip.h), field for field
RECORD = np.dtype([("temperature", "<f4"), ("top_p", "<f4"), ("top_k", "<i4"), ("stream", "<u4"), ("seed", "<u8")])
DEFAULT_TOP_K = 50      # GenerationConfig's default in the transformers range the reference pins (<= 4.42)


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """The published Philox4x32 with 10 rounds: four 32-bit counter words, two key words -> four output words."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def uniform(seed: int, stream: int, n: int) -> float:
    """u in [0, 1), a multiple of 2^-24, for token index n of request `stream` under the 64-bit `seed`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x0 = philox4x32_10((n, stream, 0, 0), (seed & _M32, seed >> 32))[0]
    return (x0 >> 8) * 2.0 ** -24


def _first_argmax(l: np.ndarray) -> int:
    return int(np.argmax(l))            # numpy returns the first maximum


def kept_mask(logits, T: float, k: int, p: float) -> np.ndarray:
    """bool [vocab]: the kept set K of the definition (T > 0)."""
    s = np.asarray(logits, np.float64) / float(T)
    V = s.shape[0]
    e = np.exp(s - s.max())
    keep = np.ones(V, bool)
    if 0 < k < V:
        keep = s >= np.partition(s, V - k)[V - k]
    if 0.0 < p < 1.0:
        ki = np.nonzero(keep)[0]
        vals, inv = np.unique(s[ki], return_inverse=True)                 # ascending distinct values
        mass = np.bincount(inv, weights=e[ki], minlength=len(vals))
        above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])  # mass of the kept values strictly greater
        keep[ki] = (above < p * e[ki].sum())[inv]
    return keep


def cdf_intervals(logits, T: float, keep: np.ndarray):
    """(idx, lo, hi): the kept indices in index order and each one's interval [lo, hi) of the cumulative distribution over K."""
    s = np.asarray(logits, np.float64) / float(T)
    idx = np.nonzero(keep)[0]
    w = np.exp(s[idx] - s.max())
    cum = np.cumsum(w)
    return idx, (cum - w) / cum[-1], cum / cum[-1]


def top_set(logits, size: int) -> Optional[np.ndarray]:
    """bool [vocab]: the `size` largest values - kept sets are nested, so a size names one - or None when ties at the edge make no
    set of exactly that size."""
    l = np.asarray(logits, np.float64)
    V = l.shape[0]
    if not 1 <= size <= V:
        return None
    keep = l >= np.partition(l, V - size)[V - size]
    return keep if int(keep.sum()) == size else None


def reference_pick(logits, T: float, k: int, p: float, seed: int, stream: int, n: int):
    """(token, |K|, (idx, lo, hi)) for one fp32 logits row; (idx, lo, hi) as `cdf_intervals` gives them for K."""
    l = np.asarray(logits, np.float64)
    if T == 0:
        tok = _first_argmax(l)
        return tok, 1, (np.array([tok]), np.array([0.0]), np.array([1.0]))
    keep = kept_mask(l, T, k, p)
    idx, lo, hi = cdf_intervals(l, T, keep)
    u = uniform(seed, stream, n)
    hit = np.nonzero(hi > u)[0]
    tok = int(idx[hit[0]]) if len(hit) else int(idx[-1])
    return tok, int(len(idx)), (idx, lo, hi)


def check_sampling(sampling: Optional[dict]) -> Optional[dict]:
    """Validated copy of a `sampling=` argument: dict(temperature, top_k=50, top_p=1.0, seed=0) or None (greedy).  transformers
    raises ValueError for the same values (temperature <= 0, top_p outside (0, 1], top_k < 0)."""
    if sampling is None:
        return None
    unknown = set(sampling) - {"temperature", "top_k", "top_p", "seed"}
    if unknown:
        raise ValueError(f"sampling: unknown keys {sorted(unknown)}")
    T, k = float(sampling.get("temperature", 1.0)), sampling.get("top_k", DEFAULT_TOP_K)
    p, seed = sampling.get("top_p", 1.0), int(sampling.get("seed", 0))
    k, p = 0 if k is None else int(k), 1.0 if p is None else float(p)
    if not (T > 0.0 and np.isfinite(T)):
        raise ValueError(f"sampling temperature must be a positive number, got {T!r} (greedy: pass sampling=None)")
    if not 0.0 < p <= 1.0:
        raise ValueError(f"sampling top_p must be in (0, 1], got {p!r}")
    if k < 0:
        raise ValueError(f"sampling top_k must be >= 0 (0 = off), got {k!r}")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"sampling seed must fit 64 bits, got {seed!r}")
    return dict(temperature=T, top_k=k, top_p=p, seed=seed)


def records(sampling: Optional[dict], streams: Sequence[int]) -> np.ndarray:
    """aur_sampling records (numpy, RECORD) for requests `streams` under one validated `sampling` dict; None = greedy records."""
    out = np.zeros(len(streams), RECORD)
    if sampling is not None:
        out["temperature"], out["top_p"], out["top_k"] = sampling["temperature"], sampling["top_p"], sampling["top_k"]
        out["seed"] = np.uint64(sampling["seed"])
        out["stream"] = np.asarray([int(s) & _M32 for s in streams], np.uint32)
    return out

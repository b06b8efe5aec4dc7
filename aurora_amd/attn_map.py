"""Which keys each generated token looked at, as this package defines it, restated in numpy.  No GPU, no torch.

Take the decode step that picks generated token i >= 1 of a sequence (token 0 is picked by the prefill and has no record).  In layer l,
head h the step's query is the roped fp16 q it wrote, and it attends to keys [0, npos) of the sequence, npos = pos + 1 - the key the
step has just written included:

    P[l, h, j] = softmax_j(scale * q_lh . k_j)  over exactly those keys        (`probabilities`; scale = 1 / sqrt(head_dim))
    A[i, j]    = mean over the selected layers l and ALL heads h of P[l, h, j]   for j < min(W, npos)
    A[i, j]    = 0.0                                                             for min(W, npos) <= j < W          (`record_row`)

W is the key window, a multiple of 64 chosen when the feature is enabled (`check_attn_map`): the prompt - and with it the visual
prefix - sits at the front of the context, so a prefix window is enough.  Row 0 of a caption and every row at or beyond its length are
zeros; with W >= npos a recorded row sums to 1.  The engine evaluates P in fp32 from the fp16 q and K the decode attention itself reads
(csrc/attn_map.hip); tests/attn_map_ref.py holds the elementwise bound between the two.

`visual` picks the columns of the visual tokens with the splice plan's `vis_rows`; `to_patches` spreads each visual token's mass evenly
over the patches it stands for (the merge map of the same run: `aurora_amd.merge_map`), a heat map over the patch grid per generated
token; `render` tiles those for the eye.  Host work, not on the hot path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

KEY_BLOCK = 64          # the window is a whole number of KV pages


def check_attn_map(attn_map, n_layers: Optional[int] = None):
    """The `attn_map=` argument of the generation calls: None (off) or dict(keys=W or None, layers=None or a list of layer indices)
    -> None or (W or None, sorted tuple of layers or None).  keys: a positive multiple of 64, None = the prompt length rounded up
    to 64 (the caller resolves it).  layers: None = all; negative indices count from the last layer when n_layers is given."""
    if attn_map is None:
        return None
    if not isinstance(attn_map, dict) or set(attn_map) - {"keys", "layers"}:
        raise ValueError(f"attn_map must be None or dict(keys=..., layers=...), got {attn_map!r}")
    keys, layers = attn_map.get("keys"), attn_map.get("layers")
    if keys is not None:
        if isinstance(keys, bool) or not isinstance(keys, (int, np.integer)) or keys < KEY_BLOCK or keys % KEY_BLOCK:
            raise ValueError(f"attn_map keys must be None or a positive multiple of {KEY_BLOCK}, got {keys!r}")
        keys = int(keys)
    if layers is not None:
        if isinstance(layers, (str, bytes)) or not hasattr(layers, "__iter__"):
            raise ValueError(f"attn_map layers must be None or a list of layer indices, got {layers!r}")
        out = []
        for l in layers:
            if isinstance(l, bool) or not isinstance(l, (int, np.integer)):
                raise ValueError(f"attn_map layers must be ints, got {l!r}")
            l = int(l)
            if n_layers is not None:
                if not -n_layers <= l < n_layers:
                    raise ValueError(f"attn_map layer {l} outside a model of {n_layers} layers")
                l %= n_layers
            elif l < 0:
                raise ValueError(f"attn_map layer {l} is negative")
            if l >= 64:
                raise ValueError(f"attn_map layer {l}: the layer mask holds layers [0, 64)")
            out.append(l)
        if not out or len(set(out)) != len(out):
            raise ValueError(f"attn_map layers must be a non-empty list without repeats, got {list(layers)!r}")
        layers = tuple(sorted(out))
    return keys, layers


def layer_mask(layers: Optional[Sequence[int]]) -> int:
    """the uint64 of aur_attn_map_enable: bit l = layer l, 0 = all"""
    return 0 if layers is None else sum(1 << int(l) for l in layers)


def window_for(prompt_len: int) -> int:
    """keys=None: the prompt length rounded up to a whole page"""
    return max(KEY_BLOCK, (int(prompt_len) + KEY_BLOCK - 1) // KEY_BLOCK * KEY_BLOCK)


def probabilities(q: np.ndarray, k: np.ndarray, scale: Optional[float] = None) -> np.ndarray:
    """q [..., hd], k [..., npos, hd] -> float64 [..., npos]: softmax_j(scale q . k_j), scale = 1 / sqrt(hd) by default"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    scale = q.shape[-1] ** -0.5 if scale is None else float(scale)
    s = np.einsum("...d,...jd->...j", q, k) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def record_row(q: np.ndarray, k: np.ndarray, window: int, scale: Optional[float] = None) -> np.ndarray:
    """One row of the record: q [layers, heads, hd] (the selected layers), k [layers, heads, npos, hd] -> float64 [window]."""
    p = probabilities(q, k, scale)
    p = p.reshape(-1, p.shape[-1]).mean(0)
    out = np.zeros(int(window), np.float64)
    n = min(int(window), p.shape[0])
    out[:n] = p[:n]
    return out


def visual(attn: np.ndarray, vis_rows) -> np.ndarray:
    """attn [n, W], vis_rows (the splice plan's: the context position of every visual token) -> [n, nvis]; a visual token at or
    beyond the window contributes 0."""
    attn, rows = np.asarray(attn), np.asarray(vis_rows, np.int64).reshape(-1)
    if attn.ndim != 2:
        raise ValueError(f"attn must be [n_tokens, window], got {attn.shape}")
    if rows.size and rows.min() < 0:
        raise ValueError("negative visual row")
    out = np.zeros((attn.shape[0], rows.size), attn.dtype)
    inside = rows < attn.shape[1]
    out[:, inside] = attn[:, rows[inside]]
    return out


def to_patches(visual_attention: np.ndarray, map_: np.ndarray) -> np.ndarray:
    """visual_attention [n, frames * n_kept] (visual tokens frame by frame, as `aur_vit_encode` returns them), map [frames, gh, gw]
    (or [frames, gh * gw]) with entries in [0, n_kept) -> float64 [n, frames, gh, gw] (or [n, frames, gh * gw]): every patch gets the
    mass of the token it was merged into divided by the number of patches in that token, so that a frame's heat map sums to the mass
    of its tokens that stand for at least one patch."""
    va, m = np.asarray(visual_attention, np.float64), np.asarray(map_)
    if va.ndim != 2 or m.ndim < 2:
        raise ValueError(f"visual_attention must be [n, nvis] and map [frames, ...], got {va.shape} and {m.shape}")
    frames = m.shape[0]
    if frames < 1 or va.shape[1] % frames:
        raise ValueError(f"{va.shape[1]} visual tokens do not divide into {frames} frames")
    n_kept = va.shape[1] // frames
    flat = m.reshape(frames, -1).astype(np.int64)
    if flat.size and (flat.min() < 0 or flat.max() >= n_kept):
        raise ValueError(f"map entries outside [0, {n_kept})")
    out = np.empty((va.shape[0], frames, flat.shape[1]), np.float64)
    for f in range(frames):
        cnt = np.bincount(flat[f], minlength=n_kept).astype(np.float64)
        per = va[:, f * n_kept:(f + 1) * n_kept] / np.maximum(cnt, 1.0)[None, :]
        out[:, f] = per[:, flat[f]]
    return out.reshape((va.shape[0],) + m.shape)


def render(heat: np.ndarray, patch: int = 8, gap: int = 1) -> np.ndarray:
    """heat [n, frames, gh, gw] -> uint8 [n * (gh * patch + gap) - gap, frames * (gw * patch + gap) - gap, 3]: one row of tiles per
    generated token, one tile per frame, each token's maps scaled by that token's largest patch value; black (cold) to white through
    red and yellow; the gaps are mid-grey."""
    h = np.asarray(heat, np.float64)
    if h.ndim != 4 or min(h.shape) < 1:
        raise ValueError(f"heat must be a non-empty [n, frames, gh, gw], got {h.shape}")
    patch, gap = int(patch), int(gap)
    if patch < 1 or gap < 0:
        raise ValueError("patch must be >= 1 and gap >= 0")
    n, frames, gh, gw = h.shape
    top = h.reshape(n, -1).max(1)
    x = np.clip(h / np.where(top > 0, top, 1.0)[:, None, None, None], 0.0, 1.0)
    rgb = np.stack([np.clip(3 * x, 0, 1), np.clip(3 * x - 1, 0, 1), np.clip(3 * x - 2, 0, 1)], -1)
    rgb = np.floor(rgb * 255 + 0.5).astype(np.uint8)
    th, tw = gh * patch, gw * patch
    out = np.full((n * (th + gap) - gap, frames * (tw + gap) - gap, 3), 128, np.uint8)
    for i in range(n):
        for f in range(frames):
            tile = np.repeat(np.repeat(rgb[i, f], patch, axis=0), patch, axis=1)
            out[i * (th + gap): i * (th + gap) + th, f * (tw + gap): f * (tw + gap) + tw] = tile
    return out

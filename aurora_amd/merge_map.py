"""Which patches each visual token stands for, as this package defines it, restated in numpy.  No GPU, no torch.

    rows = step_rows(t, unm, src, dst)          one ToMe step: old row j of a frame becomes new row rows[j]
    group = compose(t0, steps)                  the chain of steps: input row j ends in output row group[j]

A ToMe step (tome.py:36-81, class_token=True) runs over the t rows of a frame.  The even rows are the A tokens, ta = ceil(t / 2) of them,
the odd rows the B tokens; r' = len(src) = min(r, (t - 1) // 2) A tokens are merged into B tokens, and the step's output is the
ta - r' unmerged A tokens followed by the t // 2 B tokens (tome.py:81).  With the index arrays `tome_select_kernel` writes - `unm`
ascending, `src` in rank order, `dst[k]` the B token `src[k]` merges into -

  * an odd row 2 i + 1 (a B token) goes to (ta - r') + i;
  * an even row 2 unm[k] (an unmerged A token) goes to k;
  * an even row 2 src[k] (a merged A token) goes to (ta - r') + dst[k].

The chain starts at group[j] = j over the t0 = 1 + gh * gw input rows of a frame (row 0 the class token) and sets
group[j] = step_rows(...)[group[j]] behind every merging layer; a layer with r' = 0 changes nothing.  The class row is never a source
and nothing merges into it (tome.py:55-56): group[0] == 0 and group[j] >= 1 for every patch.

What the engine returns (`AuroraCapEngine.vit_encode(..., merge_map=True)`) is the chain without the class row:

  * merge_map[f][p] = group[1 + p] - 1 in [0, n_kept): the index, among the frame's kept tokens as `aur_vit_encode` returns them, of
    the token patch p was merged into; patches row-major over the gh x gw grid;
  * sizes[f][k]: the number of patches in token k - the size vector the merge kernels carry (tome.py:207-219), class entry dropped.

Three statements of the reference are this map, exactly: `merge_source`'s adjacency matrix (tome.py:222-232) is
source[f, group[j], j] = 1 (`source_matrix`); bincount(merge_map[f]) == sizes[f]; and the `unmerge` closures (tome.py:83-98) applied
from the last layer back to the first give tokens[f, merge_map[f, p], :] (`unmerge`).  tests/test_merge_map_host.py holds all three
against the reference's own results (tests/golden/g20_merge_source.npz).

`render` paints the map over the frames for the eye; it is host work and not on the hot path.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

Step = Tuple[np.ndarray, np.ndarray, np.ndarray]       # (unm, src, dst) of one layer, each [frames, .] or [.]


def clamp_r(t: int, r: int) -> int:
    """r' of a step over t rows asked to merge r (tome.py:45 with one protected token)"""
    return max(0, min(int(r), (int(t) - 1) // 2))


def step_rows(t: int, unm, src, dst, r: Optional[int] = None) -> np.ndarray:
    """int32 [t]: the new row of every old row of ONE frame.  r' = len(src); with `r` given r' = min(r, (t - 1) // 2) and only the
    first ta - r' / r' / r' entries of the arrays are read (buffers longer than the step needs)."""
    t = int(t)
    ta = (t + 1) // 2
    src, dst, unm = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1), np.asarray(unm).reshape(-1)
    rl = len(src) if r is None else clamp_r(t, r)
    nu = ta - rl
    if len(src) < rl or len(dst) < rl or len(unm) < nu:
        raise ValueError(f"a step over {t} rows with r' = {rl} needs {nu} unm and {rl} src / dst entries, "
                         f"got {len(unm)} / {len(src)} / {len(dst)}")
    rows = np.empty(t, dtype=np.int32)
    rows[1::2] = nu + np.arange(t // 2, dtype=np.int32)
    rows[2 * unm[:nu].astype(np.int64)] = np.arange(nu, dtype=np.int32)
    rows[2 * src[:rl].astype(np.int64)] = nu + dst[:rl].astype(np.int32)
    return rows


def compose(t0: int, steps: Sequence[Optional[Step]], r: Optional[int] = None) -> np.ndarray:
    """group: int32 [frames, t0] (or [t0] when the index arrays are one-dimensional): the output row every input row ends in behind
    the steps in the order given.  A step is (unm, src, dst) or None (a layer that does not merge).  `r`: see step_rows."""
    frames, flat = 1, True
    for st in steps:
        if st is not None:
            a = np.asarray(st[1])
            flat = a.ndim == 1
            frames = 1 if flat else a.shape[0]
            break
    group = np.tile(np.arange(int(t0), dtype=np.int32), (frames, 1))
    t = int(t0)
    for st in steps:
        if st is None:
            continue
        unm, src, dst = (np.asarray(a).reshape(frames, -1) for a in st)
        rl = src.shape[1] if r is None else clamp_r(t, r)
        if rl == 0:
            continue
        for f in range(frames):
            group[f] = step_rows(t, unm[f], src[f], dst[f], r)[group[f]]
        t -= rl
    return group[0] if flat else group


def to_map(group: np.ndarray) -> np.ndarray:
    """merge_map of a group vector: the class row dropped on both sides"""
    group = np.asarray(group)
    return (group[..., 1:] - 1).astype(np.int32)


def sizes(map_, n_kept: int) -> np.ndarray:
    """fp32 [frames, n_kept]: patches per token"""
    m = np.asarray(map_)
    m = m.reshape(m.shape[0], -1)
    return np.stack([np.bincount(row, minlength=int(n_kept))[: int(n_kept)] for row in m]).astype(np.float32)


def source_matrix(map_, n_kept: int) -> np.ndarray:
    """fp32 [frames, n_kept, n]: source[f, map[f, p], p] = 1 - `merge_source`'s matrix (tome.py:222-232) when given a group vector
    with its class row and n_kept + 1."""
    m = np.asarray(map_)
    m = m.reshape(m.shape[0], -1)
    if m.size and (m.min() < 0 or m.max() >= n_kept):
        raise ValueError(f"map entries outside [0, {n_kept})")
    out = np.zeros((m.shape[0], int(n_kept), m.shape[1]), dtype=np.float32)
    f, p = np.meshgrid(np.arange(m.shape[0]), np.arange(m.shape[1]), indexing="ij")
    out[f, m, p] = 1.0
    return out


def unmerge(tokens, map_) -> np.ndarray:
    """tokens [frames, n_kept, d], map [frames, ...] -> [frames, ..., d]: every patch gets the row of the token it was merged into -
    the reference's `unmerge` closures applied last layer first."""
    tokens, m = np.asarray(tokens), np.asarray(map_)
    if tokens.ndim != 3 or m.ndim < 2 or m.shape[0] != tokens.shape[0]:
        raise ValueError(f"tokens must be [frames, n_kept, d] and map [frames, ...], got {tokens.shape} and {m.shape}")
    if m.size and (m.min() < 0 or m.max() >= tokens.shape[1]):
        raise ValueError(f"map entries outside [0, {tokens.shape[1]})")
    return np.stack([tokens[f][m[f]] for f in range(m.shape[0])])


def render(frames_uint8, map_, patch: int, line=(255, 255, 255)) -> np.ndarray:
    """frames uint8 [F, H, W, 3], map [F, gh, gw] -> uint8 [F, gh * patch, gw * patch, 3].  Every patch is filled with the mean colour
    (per channel, rounded half up) of ALL pixels of its group; where two neighbouring patches belong to different groups the first
    pixel row (column) of the lower (right) one is drawn in `line`.  Pixels beyond gh * patch / gw * patch are cut, as the patch
    embedding cuts them."""
    fr, m = np.asarray(frames_uint8), np.asarray(map_)
    if fr.ndim != 4 or fr.shape[-1] != 3 or fr.dtype != np.uint8:
        raise ValueError(f"frames must be uint8 [F, H, W, 3], got {fr.dtype} {fr.shape}")
    if m.ndim != 3 or m.shape[0] != fr.shape[0]:
        raise ValueError(f"map must be [F, gh, gw] with F = {fr.shape[0]}, got {m.shape}")
    F, gh, gw = m.shape
    patch = int(patch)
    if patch < 1 or fr.shape[1] < gh * patch or fr.shape[2] < gw * patch:
        raise ValueError(f"frames of {fr.shape[1]}x{fr.shape[2]} pixels do not hold a {gh}x{gw} grid of {patch}-pixel patches")
    if m.size and m.min() < 0:
        raise ValueError("negative map entry")
    out = np.empty((F, gh * patch, gw * patch, 3), dtype=np.uint8)
    for f in range(F):
        g = m[f].reshape(-1).astype(np.int64)
        px = fr[f, : gh * patch, : gw * patch].reshape(gh, patch, gw, patch, 3).astype(np.int64)
        psum = px.sum(axis=(1, 3)).reshape(gh * gw, 3)
        n = int(g.max()) + 1
        gsum = np.zeros((n, 3), dtype=np.int64)
        np.add.at(gsum, g, psum)
        cnt = np.bincount(g, minlength=n).astype(np.int64) * patch * patch
        mean = np.floor(gsum / np.maximum(cnt, 1)[:, None] + 0.5).astype(np.uint8)
        img = np.repeat(np.repeat(mean[g].reshape(gh, gw, 3), patch, axis=0), patch, axis=1)
        mg = m[f]
        for y, x in zip(*np.nonzero(mg[1:] != mg[:-1])):               # the patch below differs
            img[(y + 1) * patch, x * patch:(x + 1) * patch] = line
        for y, x in zip(*np.nonzero(mg[:, 1:] != mg[:, :-1])):         # the patch to the right differs
            img[y * patch:(y + 1) * patch, (x + 1) * patch] = line
        out[f] = img
    return out

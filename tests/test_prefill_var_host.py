"""Host side of the variable-length prefill (no device): the C ABI carries the four `_var` entry points, the padded splice plan
scatters exactly the rows of the exact one, `caption_batch` groups by stride, the front-end bucket key does not depend on the exact
prompt length inside a bucket, and what the kernels cannot check is rejected on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

from aurora_amd import _lib
from aurora_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAR = {
    "aur_llm_prefill_batch_var": ["aur_ctx*", "int32_t", "int32_t", "void*", "int32_t", "const int32_t*", "void*"],
    "aur_llm_prefill_stage_var": ["aur_ctx*", "int32_t", "int32_t", "void*", "int32_t", "const int32_t*", "void*"],
    "aur_llm_prefill_commit_var": ["aur_ctx*", "int32_t", "int32_t", "int32_t", "void*", "int32_t", "const int32_t*", "void*"],
    "aur_project_splice_var": ["aur_ctx*", "const void*", "int32_t", "const int32_t*", "const int32_t*", "const int32_t*", "int32_t",
                               "int32_t", "void*", "void*"],
}
CT = {"int32_t": ctypes.c_int32}          # every pointer is passed as c_void_p by the binding


def test_var_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "aurora_hip.h")).read()
    assert os.path.exists(_lib.SO_PATH), "run `python -m aurora_amd.build`"
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name, want in VAR.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/aurora_hip.h"
        types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]
        assert types == want, (name, types)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == [CT.get(t, ctypes.c_void_p) for t in want], name
        assert hasattr(raw, name), f"{name} is not exported by the built library"


def scatter(plan, stride):
    """numpy emulation of the splice's two scatters: which row takes which source (visual row k -> -(k + 1), text -> its id)"""
    out = np.zeros(stride, np.int64)
    hit = np.zeros(stride, bool)
    for k, r in enumerate(plan["vis_rows"]):
        assert 0 <= r < stride and not hit[r]
        out[r], hit[r] = -(k + 1), True
    for tid, r in zip(plan["text_ids"], plan["text_rows"]):
        if r < 0:
            continue                                    # the sentinel: an unused entry of the padded plan
        assert r < stride and not hit[r]
        out[r], hit[r] = tid, True
    return out, hit


@pytest.mark.parametrize("ids,frames", [
    ([1, 5, 6, 7], 2),                                  # no marker
    ([1, -200, 9], 1),                                  # one
    ([1, 17, -200, 30, -200, 31, -200, 32, 40, 41], 3),    # several
    ([1, -200, 30, -200, 31, -200, 32, 40], 2),         # a marker beyond the frames is dropped
    ([-200, -200], 1),                                  # no text at all
])
def test_padded_splice_plan_scatters_the_rows_of_the_exact_plan(ids, frames):
    n_kept = 5
    exact = E.splice_rows(ids, frames, n_kept)
    for cap in (exact["ntext"], exact["ntext"] + 1, E._rup(max(exact["ntext"], 1), 64)):
        pad = E.splice_rows(ids, frames, n_kept, ntext_cap=cap)
        assert len(pad["text_ids"]) == len(pad["text_rows"]) == cap and pad["ntext"] == exact["ntext"] and pad["ntext_cap"] == cap
        assert (pad["text_rows"][exact["ntext"]:] == -1).all()
        assert {k: pad[k] for k in ("seq_len", "used", "nvis")} == {k: exact[k] for k in ("seq_len", "used", "nvis")}
        stride = E.prompt_stride(exact["seq_len"], 64)
        a, ha = scatter(exact, stride)
        b, hb = scatter(pad, stride)
        assert (a == b).all() and (ha == hb).all() and ha[:exact["seq_len"]].all() and not ha[exact["seq_len"]:].any()
    if exact["ntext"]:
        with pytest.raises(ValueError):
            E.splice_rows(ids, frames, n_kept, ntext_cap=exact["ntext"] - 1)


def test_prefill_groups_cover_every_clip_once_in_order_by_equal_stride():
    rng = np.random.default_rng(5)
    for bucket in E.PROMPT_BUCKETS:
        for pg in (1, 3, 8):
            lens = [int(x) for x in rng.integers(1, 400, 40)] + [64, 64, 64, 65, 128, 127, 129]
            groups = E.prefill_groups(lens, pg, bucket)
            assert [b for b, _, _ in groups] == list(np.cumsum([0] + [g for _, g, _ in groups[:-1]]))
            assert sum(g for _, g, _ in groups) == len(lens)
            for i, (b, g, st) in enumerate(groups):
                assert 1 <= g <= pg
                assert all(E.prompt_stride(x, bucket) == st for x in lens[b:b + g])
                if bucket:
                    assert st % bucket == 0 and all(st - bucket < x <= st for x in lens[b:b + g])
                if i + 1 < len(groups) and g < pg:            # a pass ends early only where the next clip's stride differs
                    assert groups[i + 1][2] != st


def test_bucket_zero_reproduces_the_equal_length_groups():
    """today's rule, restated: neighbours share a pass while their spliced lengths are equal - on the clips of the GPU suite"""
    from tests.test_gpu_caption_batch import clips
    lens = [E.splice_rows(ids, px.shape[0], 7)["seq_len"] for px, ids in clips(12, 3)]
    for pg in (1, 2, 8):
        want, b = [], 0
        while b < len(lens):
            g = 1
            while b + g < len(lens) and g < pg and lens[b + g] == lens[b]:
                g += 1
            want.append((b, g, lens[b]))
            b += g
        assert E.prefill_groups(lens, pg, 0) == want
    assert E.prefill_groups([7, 7, 7, 9, 9, 7], 2, 0) == [(0, 2, 7), (2, 1, 7), (3, 2, 9), (5, 1, 7)]


def test_front_end_key_ignores_the_prompt_length_inside_a_bucket():
    def key(ntext, bucket, seq=4):
        ids = [1] + [-200, 30] * 3 + list(range(100, 100 + ntext))
        return E.front_end_bucket_key(0, 16, 3, 56, 56, 2, seq, E.splice_rows(ids, 3, 7), bucket)
    # 3 frames x 7 rows + 4 text = 25 positions before the tail: tails 1 .. 39 stay within 64 positions and 64 text tokens
    inside = {key(n, 64) for n in range(1, 40)}
    assert len(inside) == 1
    assert key(39, 64) != key(40, 64)                       # 65 positions: the next stride
    assert len({key(n, 0) for n in range(1, 40)}) == 39     # exact lengths: a key per prompt
    assert key(5, 64) != key(5, 64, seq=5) and key(5, 64) != key(5, 32) and key(5, 64) != key(5, 0)
    k = key(5, 64)
    assert k[7] == 64 and k[10] == 64 and k[7] % 32 == 0
    # the text capacity alone can cross a bucket boundary (few visual rows, long text)
    long_text = E.front_end_bucket_key(0, 16, 0, 56, 56, 2, 4, E.splice_rows(list(range(1, 70)), 0, 7), 64)
    assert long_text[7] == 128 and long_text[10] == 128


def test_host_side_rejections():
    assert E.check_seq_lens([97, 128, 65], 128, 16, 512) == [97, 128, 65]
    for lens, stride, max_new, max_ctx in [([129], 128, 16, 512), ([0], 128, 16, 512), ([100], 100, 16, 512), ([500], 512, 16, 512)]:
        with pytest.raises(ValueError):
            E.check_seq_lens(lens, stride, max_new, max_ctx)
    for b in (0, 32, 64, 128):
        assert E.check_prompt_bucket(b) == b
    for b in (-32, 16, 48, 96, 256, None, "64"):
        with pytest.raises(ValueError):
            E.check_prompt_bucket(b)
    with pytest.raises(ValueError):                         # the bucket is checked before the engine asks for a GPU
        E.AuroraCapEngine({"vit": None, "llm": None}, {}, prompt_bucket=48)
    from aurora_amd.lmms_plugin.models.auroracap_mi355x import AuroraCapMI355X, PROMPT_BUCKET_DEFAULT
    assert PROMPT_BUCKET_DEFAULT in (0, 64)
    with pytest.raises(ValueError):
        AuroraCapMI355X(prompt_bucket=48, _model=object(), _tokenizer=object(), _preprocessor=object())

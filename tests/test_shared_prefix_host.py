"""Host side of the shared visual prefix (no device): where two splice plans stop being identical and where a sibling prompt forks,
the adaptor's sibling ordering / one preprocessing per video with an injected fake model, and the four new C entry points in the
header, the binding and the cross-compiled library."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from aurora_amd import _lib
from aurora_amd import engine as E
from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
from tests.test_lmms_plugin import FakeTok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = E.IMAGE_TOKEN_INDEX


# ---------------------------------------------------------------------------------------------------------- plans
def plan(ids, frames, n_kept=5):
    return E.splice_rows(ids, frames, n_kept)


def by_hand(vis_rows, text):
    """a plan written out row by row: text = {row: id}"""
    rows = sorted(text)
    return dict(seq_len=len(vis_rows) + len(text), used=1, nvis=len(vis_rows), vis_rows=np.asarray(vis_rows, np.int32),
                text_rows=np.asarray(rows, np.int32), text_ids=np.asarray([text[r] for r in rows], np.int32))


def test_fork_point_is_whole_pages():
    assert [E.fork_point(x) for x in (-3, 0, 1, 63, 64, 65, 127, 128, 2141)] == [0, 0, 0, 0, 64, 64, 64, 128, 2112]
    assert E.FORK_TOKENS == 64


def test_equal_visuals_with_different_tails():
    head = [1, 7] + [IMG, 30] * 3
    a, b = plan(head + [40, 41, 42], 3), plan(head + [40, 50], 3)
    assert a["seq_len"] == 2 + 3 * 6 + 3 and E.shared_prefix_rows(a, b) == E.shared_prefix_rows(b, a) == 2 + 3 * 6 + 1
    assert E.shared_prefix_rows(a, plan(head, 3)) == 20                       # one is a prefix of the other: its whole length
    # 13 frames of 5 rows: 1 + 13 * 6 = 79 common rows -> the fork is the page below, and the child keeps its tail
    head = [1] + [IMG, 30] * 13
    a, b = plan(head + [40] * 60, 13), plan(head + [40] * 50 + [41] * 3, 13)
    assert E.shared_prefix_rows(a, b) == 79 + 50 and E.share_fork(a, b) == 128 and E.share_fork(b, a) == 128
    assert E.share_fork(a, plan(head + [41], 13)) == 64


def test_different_frame_counts():
    a, b = plan([1] + [IMG, 30] * 3 + [40], 3), plan([1] + [IMG, 30] * 4 + [40], 4)
    assert E.shared_prefix_rows(a, b) == 1 + 3 * 6                            # b's fourth frame stands where a's text goes on
    assert E.share_fork(a, b) == 0 and E.share_fork(b, a) == 0               # not the same visual input, whatever the key said
    big_a, big_b = plan([1] + [IMG, 30] * 13 + [40], 13), plan([1] + [IMG, 30] * 14 + [40], 14)
    assert E.shared_prefix_rows(big_a, big_b) == 79 and E.share_fork(big_a, big_b) == 0
    # a marker beyond the frames is dropped: the same rows as without it
    assert E.shared_prefix_rows(plan([1, IMG, 30, IMG, 31], 1), plan([1, IMG, 30, 31], 1)) == 8


def test_divergence_inside_the_system_text():
    sys_a, sys_b = [1, 11, 12, 13, 14], [1, 11, 12, 99, 14]
    a, b = plan(sys_a + [IMG, 30] * 13 + [40], 13), plan(sys_b + [IMG, 30] * 13 + [40], 13)
    assert E.shared_prefix_rows(a, b) == 3
    assert E.share_fork(a, b) == 0                                            # diverges before the visual rows end: never shared
    # text in FRONT of the visual rows long enough for a page: still no fork, the visual rows would not be covered
    long_a, long_b = plan(list(range(1, 81)) + [IMG, 30] * 2 + [40], 2), plan(list(range(1, 81)) + [IMG, 31] * 2 + [40], 2)
    assert E.shared_prefix_rows(long_a, long_b) == 80 + 5 and E.share_fork(long_a, long_b) == 0


def test_identical_prompts_keep_a_row_of_their_own():
    ids = [1] + [IMG, 30] * 13 + [40] * 49                                    # 79 + 49 = 128 rows: exactly two pages
    a = plan(ids, 13)
    assert a["seq_len"] == 128 and E.shared_prefix_rows(a, a) == 128
    assert E.share_fork(a, a) == 64                                           # not 128: the first token comes from the child's own last row
    b = plan(ids + [41], 13)
    assert E.share_fork(a, b) == 128 and E.share_fork(b, a) == 64
    short = plan([1] + [IMG, 30] * 2 + [40], 2)
    assert E.share_fork(short, short) == 0                                    # less than a page: the fork point is 0, no sharing
    assert E.share_fork(plan([1, 2, 3] * 30, 0), plan([1, 2, 3] * 30, 0)) == 0      # no visual rows at all


def test_hand_built_plans_and_the_rows_they_describe():
    a = by_hand([1, 2, 3], {0: 1, 4: 30, 5: 40})
    b = by_hand([1, 2, 3], {0: 1, 4: 30, 5: 41, 6: 42})
    c = by_hand([2, 3, 4], {0: 1, 1: 9, 5: 30})
    assert E.shared_prefix_rows(a, b) == 5 and E.shared_prefix_rows(a, c) == 1 and E.shared_prefix_rows(a, a) == 6
    # the same VISUAL ROW INDEX, not just "a visual row": row 2 is visual row 1 in a and visual row 0 in c
    d = by_hand([1, 2, 3], {0: 1, 4: 31})
    assert E.shared_prefix_rows(a, d) == 4
    # splice_rows' own description agrees with the arrays it returns
    p = plan([1, 17, IMG, 30, IMG, 31, 40], 2)
    assert (p["row_src"] == E._row_sources({k: p[k] for k in ("seq_len", "vis_rows", "text_rows", "text_ids")})).all()
    pad = E.splice_rows([1, 17, IMG, 30, IMG, 31, 40], 2, 5, ntext_cap=64)
    assert E.shared_prefix_rows(p, pad) == p["seq_len"] and pad["vis_end"] == p["vis_end"] == 13


def test_extend_lengths_are_checked_against_the_position_they_start_at():
    assert E.check_seq_lens([1, 33], 64, 16, 512, 128) == [1, 33]
    with pytest.raises(ValueError):
        E.check_seq_lens([40], 64, 16, 512, 512 - 16 - 39)
    assert E.check_seq_lens([40], 64, 16, 512, 512 - 16 - 40) == [40]
    with pytest.raises(ValueError):
        E.AuroraCapEngine({"vit": None, "llm": None}, {}, spare_slots=1, prefix_cache=2)      # checked before the engine asks for a GPU


def test_holder_cache_is_least_recently_used():
    h = E._PrefixHolders([7, 8])
    assert h.get("a") is None
    assert {h.put("a", x=1)["seq"], h.put("b", x=2)["seq"]} == {7, 8}
    seq_a = h.get("a")["seq"]                                                 # touch a: b is now the oldest
    assert h.put("c", x=3)["seq"] != seq_a and h.get("b") is None and h.get("a")["x"] == 1
    assert h.put("a", x=4)["seq"] == seq_a and h.get("a")["x"] == 4          # the same key keeps its sequence
    assert E._PrefixHolders([]).put("a") is None


# ---------------------------------------------------------------------------------------------------------- adaptor
class StreamModel:
    """records the order in which the stream pulls its clips and the key each position gets"""

    def __init__(self, with_stream=True):
        self.visual_encoder = SimpleNamespace(reset_tome_r=lambda r: None)
        self.pulled, self.keys, self.kw = [], [], []
        if not with_stream:
            self.caption_stream = None
            del self.caption_stream

    def caption_stream(self, clips, max_new_tokens=2048, on_error=None, share_key=None, **kw):
        self.kw.append(dict(kw, share_key=share_key is not None))
        for k, (px, ids) in enumerate(clips):
            self.pulled.append((px, ids))
            self.keys.append(share_key(k) if share_key is not None else None)
            yield k, [int(px[0, 0, 0, 0]), len(ids)]


def adaptor(model, **kw):
    m = P.AuroraCapMI355X(pretrained="unused", device="cpu", batch_size=4, _model=model, _tokenizer=FakeTok(), **kw,
                          _preprocessor=lambda fr: torch.full((fr.shape[0], 3, 2, 2), float(fr[0, 0, 0, 0]), dtype=torch.float16))
    m.loads = []

    def load_frames(visuals):                                                 # "video 3.mp4" decodes to 2 frames filled with 3
        m.loads.append(tuple(visuals))
        return np.full((2, 4, 4, 3), int(re.search(r"(\d+)", visuals[0]).group(1)), np.uint8)
    m.load_frames = load_frames
    return m


def vdc_requests(n_videos=4, questions=("short?", "a much longer question about the background?", "camera?")):
    """what lmms-eval hands over for several tasks over one dataset: task-major, every task asks about every video"""
    docs = {v: f"video {v}.mp4" for v in range(n_videos)}
    reqs = [SimpleNamespace(args=(q, {}, lambda d: [d], v, "vdc", "test")) for q in questions for v in range(n_videos)]
    return docs, reqs


def test_visual_key():
    assert P.visual_key(["a.mp4"]) == ("a.mp4",) and P.visual_key(["a.png", "b.png"]) == ("a.png", "b.png")
    assert P.visual_key([{"video_path": "a.mp4", "keyframe": [0.5, 2]}]) == ("a.mp4", (0.5, 2))
    assert P.visual_key([np.zeros((2, 4, 4, 3))]) is None and P.visual_key([]) is None and P.visual_key(["a.mp4", 3]) is None
    assert P.visual_key([SimpleNamespace(convert=lambda m: None)]) is None   # a PIL image


def test_group_siblings_is_a_stable_sort_by_first_occurrence():
    keys = {0: "x", 1: None, 2: "y", 3: "x", 4: None, 5: "y", 6: "x"}
    assert P.group_siblings([0, 1, 2, 3, 4, 5, 6], keys.get) == [0, 3, 6, 1, 2, 5, 4]
    assert P.group_siblings([5, 4, 3], keys.get) == [5, 4, 3]
    assert P.group_siblings([], keys.get) == []


def test_adaptor_makes_siblings_neighbours_and_preprocesses_each_video_once():
    docs, reqs = vdc_requests()
    model = StreamModel()
    m = adaptor(model, share_visual_prefix=True)
    m.task_dict = {"vdc": {"test": docs}}
    out = m.generate_until(reqs)
    vids = [int(px[0, 0, 0, 0]) for px, _ in model.pulled]
    assert len(vids) == 12 and all(vids[i] == vids[i - i % 3] for i in range(12)) and sorted(set(vids)) == [0, 1, 2, 3]      # runs of 3
    assert model.keys == [(f"video {v}.mp4",) for v in vids]
    assert len(m.loads) == 4 and sorted(m.loads) == [(f"video {v}.mp4",) for v in range(4)]           # decoded and preprocessed once per key
    assert all(model.pulled[i][0] is model.pulled[i - i % 3][0] for i in range(12))                  # the very same pixel tensor
    assert model.kw == [dict(share_key=True)]                                                          # no overlap= for an injected model
    tok = FakeTok()
    for r, text in zip(reqs, out):                                             # every result belongs to ITS request
        ids = P.tokenizer_image_token(P.conv_prompt(P.question_with_image_tokens(r.args[0], 2)), tok)
        assert text == f"{r.args[3]} {len(ids)}"
    # the order inside a video's run is the order plan_batches gave (longest prompt first)
    lens = [len(ids) for _, ids in model.pulled]
    assert all(lens[i] >= lens[i + 1] for i in range(12) if i % 3 != 2)


def test_adaptor_without_sharing_keeps_the_order_of_plan_batches():
    docs, reqs = vdc_requests()
    model = StreamModel()
    m = adaptor(model)
    assert m.share_visual_prefix is False
    m.task_dict = {"vdc": {"test": docs}}
    out = m.generate_until(reqs)
    want = P.plan_batches([r.args for r in reqs], lambda s: len(m.tok_encode(s)), len(reqs))
    assert len(want) == 1
    assert [int(px[0, 0, 0, 0]) for px, _ in model.pulled] == [reqs[i].args[3] for i in want[0]]
    assert model.keys == [None] * 12 and model.kw == [dict(share_key=False)] and len(m.loads) == 12
    assert [t.split()[0] for t in out] == [str(r.args[3]) for r in reqs]
    for flag, val in (("true", True), ("0", False), (True, True)):
        assert adaptor(StreamModel(), share_visual_prefix=flag).share_visual_prefix is val


def test_adaptor_shares_through_caption_batch_when_the_model_has_no_stream():
    docs, reqs = vdc_requests(n_videos=2, questions=("a?", "bb?"))
    calls = []

    class BatchModel:
        visual_encoder = SimpleNamespace(reset_tome_r=lambda r: None)

        def caption_batch(self, clips, max_new_tokens=2048, share=None):
            calls.append(share)
            return [[int(px[0, 0, 0, 0]), len(ids)] for px, ids in clips]
    m = adaptor(BatchModel(), share_visual_prefix=True)
    m.task_dict = {"vdc": {"test": docs}}
    out = m.generate_until(reqs)
    assert len(calls) == 1 and calls[0][0] == calls[0][1] and calls[0][2] == calls[0][3] and calls[0][0] != calls[0][2]
    assert [t.split()[0] for t in out] == [str(r.args[3]) for r in reqs] and len(m.loads) == 2


# ---------------------------------------------------------------------------------------------------------- C ABI
NEW = {
    "aur_kv_copy_prefix": ["aur_ctx*", "int32_t", "int32_t", "int32_t", "int32_t", "void*"],
    "aur_llm_extend_batch_var": ["aur_ctx*", "int32_t", "int32_t", "void*", "int32_t", "int32_t", "const int32_t*", "void*"],
    "aur_llm_extend_stage_var": ["aur_ctx*", "int32_t", "int32_t", "void*", "int32_t", "int32_t", "const int32_t*", "void*"],
    "aur_llm_extend_commit_var": ["aur_ctx*", "int32_t", "int32_t", "int32_t", "void*", "int32_t", "int32_t", "const int32_t*", "void*"],
}
CT = {"int32_t": ctypes.c_int32}          # every pointer is passed as c_void_p by the binding


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "aurora_hip.h")).read()
    assert os.path.exists(_lib.SO_PATH), "run `python -m aurora_amd.build`"
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name, want in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/aurora_hip.h"
        types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]
        assert types == want, (name, types)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == [CT.get(t, ctypes.c_void_p) for t in want], name
        assert hasattr(raw, name), f"{name} is not exported by the built library"
    # the extend calls are the _prefill_*_var calls plus `int32_t pos0` in front of the stride
    for form in ("batch", "stage", "commit"):
        old = _lib.SIGNATURES[f"aur_llm_prefill_{form}_var"][1]
        new = _lib.SIGNATURES[f"aur_llm_extend_{form}_var"][1]
        assert len(new) == len(old) + 1 and new[:-3] == old[:-2] and new[-4] is ctypes.c_int32
    assert "BITWISE those of aur_llm_prefill(slot, full_embeds_i, pos0 + len_i)" in hdr

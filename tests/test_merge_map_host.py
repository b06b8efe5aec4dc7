"""CPU: the merge map as aurora_amd/merge_map.py defines it, against what the reference's own merge module computed
(tests/golden/g20_merge_source.npz, written by tests/golden/make_golden_merge_source.py): `merge_source`'s adjacency matrix reduced to
a group vector, the size vector of `merge_wavg`, and the chain of `unmerge` closures.  Integers and copies: every comparison is exact.

The mutant test shows that the fixture can tell the rule from six near misses of it, and prints which case catches which."""
import os
import subprocess
import sys

import numpy as np
import pytest

from aurora_amd import merge_map as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g20_merge_source.npz"))
CASES = [str(c) for c in G["cases"]]


def case(name):
    frames, t0, r, layers, d = (int(v) for v in G[f"{name}_meta"])
    steps = [(G[f"{name}_L{l}_unm"], G[f"{name}_L{l}_src"], G[f"{name}_L{l}_dst"]) for l in range(layers)]
    return dict(frames=frames, t0=t0, r=r, layers=layers, d=d, steps=steps, group=G[f"{name}_group"], size=G[f"{name}_size"],
                x=G[f"{name}_x"], unmerged=G[f"{name}_unmerged"])


def test_fixture_holds_the_cases_the_definition_names():
    assert CASES == ["path15", "path22", "clamp", "tiny", "mid", "tie", "nonsquare"]
    c = case("path15")
    assert (c["frames"], c["t0"], c["layers"], c["size"].shape[1]) == (2, 730, 31, 265)
    c = case("clamp")                                     # 10 -> 6 -> 4 -> 3 -> 2 -> 2: the clamp, then a layer that does not merge
    assert [s[1].shape[1] for s in c["steps"]] == [4, 2, 1, 1, 0] and c["size"].shape[1] == 2
    assert case("nonsquare")["t0"] == 1 + 20 * 31 and case("tie")["t0"] == 9 and case("tiny")["t0"] == 17 and case("mid")["frames"] == 3


@pytest.mark.parametrize("name", CASES)
def test_compose_equals_the_reference_group(name):
    c = case(name)
    group = MM.compose(c["t0"], c["steps"])
    np.testing.assert_array_equal(group, c["group"])
    assert group.dtype == np.int32 and group.shape == (c["frames"], c["t0"])
    # the same chain told the nominal r alone (the arrays are exactly as long as each step needs)
    np.testing.assert_array_equal(MM.compose(c["t0"], c["steps"], r=c["r"]), c["group"])
    assert np.all(group[:, 0] == 0) and np.all(group[:, 1:] >= 1)              # the class row never moves, nothing merges into it


@pytest.mark.parametrize("name", CASES)
def test_bincount_equals_the_reference_size(name):
    c = case(name)
    m = MM.to_map(MM.compose(c["t0"], c["steps"]))
    n_kept = c["size"].shape[1] - 1
    assert m.min() >= 0 and m.max() < n_kept
    assert np.all(c["size"][:, 0] == 1.0)
    np.testing.assert_array_equal(MM.sizes(m, n_kept), c["size"][:, 1:])
    assert MM.sizes(m, n_kept).sum(axis=1).tolist() == [c["t0"] - 1] * c["frames"]


@pytest.mark.parametrize("name", CASES)
def test_unmerge_equals_the_reference_chain(name):
    c = case(name)
    group = MM.compose(c["t0"], c["steps"])
    got = MM.unmerge(c["x"], group)
    assert got.dtype == c["unmerged"].dtype
    np.testing.assert_array_equal(got.view(np.uint16), c["unmerged"].view(np.uint16))
    # without the class row on both sides: the form the engine returns
    np.testing.assert_array_equal(MM.unmerge(c["x"][:, 1:], MM.to_map(group)).view(np.uint16), c["unmerged"][:, 1:].view(np.uint16))


@pytest.mark.parametrize("name", CASES)
def test_source_matrix_round_trips(name):
    c = case(name)
    group = MM.compose(c["t0"], c["steps"])
    t = c["size"].shape[1]
    src = MM.source_matrix(group, t)                                            # the reference's `source` [frames, t_final, t0]
    assert src.shape == (c["frames"], t, c["t0"]) and np.all(src.sum(axis=1) == 1)
    np.testing.assert_array_equal(src.argmax(axis=1), group)
    np.testing.assert_array_equal(src.sum(axis=2), c["size"])
    m = MM.to_map(group).reshape(c["frames"], -1)
    np.testing.assert_array_equal(MM.source_matrix(m, t - 1), src[:, 1:, 1:])


def test_step_rows_by_hand():
    # t = 7: A rows 0 2 4 6 (ta = 4), B rows 1 3 5; r' = 2: src = [3, 1] (rows 6, 2) into dst = [0, 2] (rows 1, 5); unm = [0, 2]
    rows = MM.step_rows(7, [0, 2], [3, 1], [0, 2])
    assert rows.tolist() == [0, 2, 4, 3, 1, 4, 2]
    assert MM.step_rows(7, [0, 2, 9, 9], [3, 1, 9], [0, 2, 9], r=2).tolist() == rows.tolist()     # longer buffers, r given
    assert MM.step_rows(4, [0, 1], [], []).tolist() == [0, 2, 1, 3]                                 # r' = 0: A rows, then B rows
    assert MM.compose(4, [None, (np.zeros(0, int), np.zeros(0, int), np.zeros(0, int))]).tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        MM.step_rows(7, [0], [3, 1], [0, 2])
    assert [MM.clamp_r(t, 5) for t in (1, 2, 3, 10, 11, 12)] == [0, 0, 1, 4, 5, 5] and MM.clamp_r(9, -1) == 0


def test_render_on_a_hand_made_case():
    """2 x 2 patches of 2 x 2 pixels; the two patches of the top row are one group, the bottom ones a group each."""
    fr = np.zeros((1, 5, 4, 3), np.uint8)                    # a fifth pixel row that no patch covers: cut
    fr[0, 0:2, 0:2] = (10, 20, 30)
    fr[0, 0:2, 2:4] = (20, 40, 61)                           # group 0: mean (15, 30, 45.5 -> 46: half rounds up)
    fr[0, 2:4, 0:2] = (100, 0, 0)
    fr[0, 2:4, 2:4] = [[(0, 200, 0), (0, 100, 0)], [(0, 100, 0), (0, 0, 3)]]          # mean (0, 100, 0.75 -> 1)
    m = np.array([[[0, 0], [1, 2]]], np.int32)
    out = MM.render(fr, m, 2)
    assert out.shape == (1, 4, 4, 3) and out.dtype == np.uint8
    W = (255, 255, 255)
    want = np.array([[(15, 30, 46)] * 4,
                     [(15, 30, 46)] * 4,
                     [W, W, W, W],                           # the first pixel row of the lower patches: both differ from the patch above
                     [(100, 0, 0), (100, 0, 0), W, (0, 100, 1)]], np.uint8)          # the first pixel column of the right patch
    np.testing.assert_array_equal(out[0], want)
    np.testing.assert_array_equal(MM.render(fr, m, 2, line=(1, 2, 3))[0, 2, 0], (1, 2, 3))
    same = MM.render(fr, np.zeros((1, 2, 2), np.int32), 2)   # one group: one colour, no line
    assert len(np.unique(same.reshape(-1, 3), axis=0)) == 1
    for bad in (lambda: MM.render(fr.astype(np.float32), m, 2), lambda: MM.render(fr, m, 3), lambda: MM.render(fr, m[0], 2),
                lambda: MM.render(fr, -m - 1, 2)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------- six near misses of the rule
def _chain(c, step, reverse=False):
    """compose, with the step rule and the layer order open to a mutant; every step is told the case's nominal r"""
    group = np.tile(np.arange(c["t0"], dtype=np.int64), (c["frames"], 1))
    ts, t = [], c["t0"]
    for unm, src, dst in c["steps"]:
        ts.append(t)
        t -= src.shape[1]
    order = list(zip(ts, c["steps"]))
    for t, (unm, src, dst) in (reversed(order) if reverse else order):
        for f in range(c["frames"]):
            group[f] = step(t, unm[f], src[f], dst[f], c["r"])[group[f]]
    return group


def _rule(t, unm, src, dst, r, *, rank_unm=False, b_off_ta=False, dst_plain=False, swap=False, no_clamp=False):
    ta = (t + 1) // 2
    rl = r if no_clamp else min(r, (t - 1) // 2)
    nu = ta - rl
    if rank_unm:                  # the one certain trait of rank order: the class row's score is -inf, so it comes LAST, not first
        unm = np.roll(unm, -1)
    even, odd = (1, 0) if swap else (0, 1)
    rows = np.zeros(t + 1, dtype=np.int64)
    rows[odd:t:2][: t // 2] = (ta if b_off_ta else nu) + np.arange(t // 2)
    rows[2 * unm.astype(np.int64) + even] = np.arange(len(unm))
    rows[2 * src.astype(np.int64) + even] = (0 if dst_plain else nu) + dst
    return rows[:t]


MUTANTS = {
    "1 unm in rank order, not ascending": dict(rank_unm=True),
    "2 B rows offset by ta, not ta - r'": dict(b_off_ta=True),
    "3 dst without the offset": dict(dst_plain=True),
    "4 even and odd rows swapped": dict(swap=True),
    "5 the (t - 1) // 2 clamp dropped": dict(no_clamp=True),
    "6 layers composed in reverse order": dict(reverse=True),
}


def test_six_mutants_of_step_rows_are_each_caught_by_a_fixture_case():
    for name in CASES:                                       # the harness itself, unmutated, is the rule
        c = case(name)
        np.testing.assert_array_equal(_chain(c, _rule), c["group"])
    for label, kw in MUTANTS.items():
        kw = dict(kw)
        reverse = kw.pop("reverse", False)
        caught = []
        for name in CASES:
            c = case(name)
            try:
                got = _chain(c, lambda *a: _rule(*a, **kw), reverse=reverse)
                if not np.array_equal(got, c["group"]):
                    caught.append(name)
            except (IndexError, ValueError):                 # a mutant that leaves its table is caught as well
                caught.append(name + " (raises)")
        print(f"mutant {label}: caught by {', '.join(caught) if caught else 'NOTHING'}")
        assert caught, label
        if "clamp" in label:                                 # what only ONE case can see
            assert [n.split()[0] for n in caught] == ["clamp"], caught


# ---------------------------------------------------------------------------------------------- arguments, no device
def test_definition_rejects_bad_arguments():
    x = np.zeros((2, 3, 8), np.float16)
    with pytest.raises(ValueError):
        MM.unmerge(x, np.array([[0, 3], [0, 0]]))            # entry outside [0, n_kept)
    with pytest.raises(ValueError):
        MM.unmerge(x, np.array([0, 1]))                      # no frame axis
    with pytest.raises(ValueError):
        MM.unmerge(x[0], np.array([[0, 1]]))
    with pytest.raises(ValueError):
        MM.source_matrix(np.array([[0, 5]]), 3)
    assert MM.unmerge(x, np.zeros((2, 4, 5), np.int32)).shape == (2, 4, 5, 8)


def test_engine_wrappers_check_their_arguments_before_the_device():
    import torch
    from aurora_amd.engine import AuroraCapEngine as E
    rows = torch.zeros(2, 4, dtype=torch.int32)
    idx = torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="on the device"):
        E.tome_map_rows(None, rows, 5, 1, idx, idx, idx)                         # host memory
    with pytest.raises(ValueError, match="on the device"):
        E.tome_map_rows(None, rows.long(), 5, 1, idx, idx, idx)
    with pytest.raises(ValueError, match="multiple of 8"):
        E.unmerge(None, torch.zeros(1, 3, 20, dtype=torch.float16), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="integer"):
        E.unmerge(None, torch.zeros(1, 3, 16, dtype=torch.float16), torch.zeros(1, 4))
    with pytest.raises(ValueError, match="integer"):
        E.unmerge(None, torch.zeros(2, 3, 16, dtype=torch.float16), torch.zeros(1, 4, dtype=torch.int32))   # frames differ
    with pytest.raises(ValueError):
        E.unmerge(None, torch.zeros(3, 16, dtype=torch.float16), torch.zeros(1, 4, dtype=torch.int32))


def test_cli_flags_exist_and_refuse_what_they_do_not_go_with():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--merge_map" in out.stdout and "--merge_vis" in out.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--merge_map", "x.npz", "--score", "a"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--merge_map" in bad.stderr

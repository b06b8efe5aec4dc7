"""Classifier-free guidance, reference side (no GPU): the fp32 restatement of the kernel's arithmetic (tests/guidance_ref.py) stays
inside the derived bound of the float64 definition on every shared case, and each of ten single mistakes leaves that bound by more than
a factor of ten - so the GPU suites, which hold the kernels to the same bound on the same kinds of rows, would see them."""
import numpy as np
import pytest

from aurora_amd import guidance as GD
from tests import guidance_ref as R

CASES = R.cases()


def test_the_bound_is_small_against_the_rows_and_grows_with_the_scale():
    for tag, c, u, g in CASES:
        b = R.bound(c, u, g)
        assert 0 < b < 2e-3, (tag, b)                           # a top-2 margin of a model row is >> this
    c, u = CASES[0][1], CASES[0][2]
    assert R.bound(c, u, 0.5) < R.bound(c, u, 1.5) < R.bound(c, u, 3.0) < R.bound(c, u, 7.5)


def test_the_fp32_restatement_stays_inside_the_derived_bound():
    worst = 0.0
    for tag, c, u, g in CASES:
        got, want = R.kernel_apply(c, u, g), GD.apply(c, u, g)
        assert got.dtype == np.float32 and np.isfinite(got).all(), tag
        ratio = float(np.abs(got.astype(np.float64) - want).max()) / R.bound(c, u, g)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (tag, ratio)
    print(f"worst error / bound over {len(CASES)} cases: {worst:.3f}")


def test_the_tree_sum_is_a_sum():
    rng = np.random.default_rng(3)
    for V in (1, 5, 1003, 4096, 4097, 32000):
        e = rng.random(V).astype(np.float32)
        assert abs(float(R.tree_sum(e)) - float(e.astype(np.float64).sum())) <= R.depth(V) * R.U * float(e.astype(np.float64).sum())


@pytest.mark.parametrize("name", sorted(R.ROW_MISTAKES))
def test_a_single_mistake_in_the_row_leaves_the_bound_tenfold(name):
    fn = R.ROW_MISTAKES[name]
    seen = 0
    for tag, c, u, g in CASES:
        if "identical" in tag and name not in ("g_lc_minus_lu", "sum_without_shift", "raw_u", "no_log_softmax"):
            continue                                            # c == u: lc - lu = 0 and both rows share m and S, so these variants are the definition
        if name == "rows_swapped" and g == 0.5:
            continue                                            # 0.5 lc + 0.5 lu is symmetric in the two rows
        err = float(np.abs(fn(c, u, g) - GD.apply(c, u, g)).max())
        assert err > 10 * R.bound(c, u, g), (name, tag, err, R.bound(c, u, g))
        seen += 1
    assert seen >= len(CASES) // 2


def test_guidance_after_the_repetition_penalty_leaves_the_bound_tenfold():
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=0, min_new_tokens=0)
    for tag, c, u, g in CASES:
        if "identical" in tag:
            continue
        top = np.argsort(c)[-3:].tolist()                        # the history holds likely tokens, as a generation's does
        right = R.chain(c, u, g, top, rules, None)
        wrong = R.chain(c, u, g, top, rules, None, guidance_first=False)
        assert float(np.abs(right - wrong).max()) > 10 * 1.3 * R.bound(c, u, g), tag


def test_the_partners_row_left_guided_leaves_the_bound_tenfold():
    rng = np.random.default_rng(11)
    for V in (1003, 32000):
        rows = np.stack([x for _ in range(2) for x in R.row_pair(rng, V)])          # rows 0 / 2 lead, 1 / 3 are their partners
        for g in R.SCALES:
            recs = GD.records(g, [(0, 1), (2, 3)], 4)
            want, save = R.apply_rows(rows, recs)
            assert np.array_equal(want[1], rows[1].astype(np.float64)) and np.array_equal(save[0], rows[0].astype(np.float64))
            assert np.isnan(save[1]).all() and np.isnan(save[3]).all()
            wrong = want.copy()
            wrong[1] = want[0]                                   # the mistake: the guided row written to the partner as well
            b = max(R.bound(rows[0], rows[1], g), R.bound(rows[2], rows[3], g))
            assert float(np.abs(wrong - want).max()) > 10 * b
            # and a launch over a part of the buffer touches nothing outside it
            part, _ = R.apply_rows(rows, recs, 2, 2)
            assert np.array_equal(part[:2], rows[:2].astype(np.float64)) and np.array_equal(part[2], want[2])

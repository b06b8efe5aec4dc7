"""CPU: the reference side of tests/test_gpu_skinny_modes.py checks itself.  The emulator of the decode projections' arithmetic
(tests/skinny_ref.py emulate) must stay inside the derived bound on every case and shape, and every mutant of it - the ways these
epilogues can be subtly wrong - must leave the bound by at least 10x on at least one case of EVERY shape it applies to, so that the
GPU test, which asserts error <= 1.0 x bound, cannot pass a kernel with one of these defects.

Results (this module prints them; `pytest -s`), 165 shapes of 4 live rows, K in {128, 256, 1152, 2304, 4224}:
  emulator, worst error / bound:  SK_ROW 0.95 (output and sum(x^2)), SK_SILU_MUL 0.97, SK_LOGITS 0.035 (an fp32 output: only the K 2^-24
  accumulation term, a worst case the actual summation trees stay far inside).
  smallest margin of each mutant over the shapes it applies to (x bound):
    rstd_over_n 717          no_eps 9.1e5              slot_dropped 64           tile_ssq_dropped 2.0e5
    ssq_unrounded 175        resid_rounded_first 30    no_resid 4.0e3            gate_up_swapped 1.1e3
    partial_dropped 1.1e3    ragged_dropped 103        dead_leak 1.0e7           n4_overflow 2.6e3
  resid_rounded_first changes an output by at most 2^-12 |y| while the accumulation term alone is K 2^-24 |y| or more: it applies to
  K <= 256 only (skinny_ref.applies); at larger K no elementwise bound of this form can see it.  The case "aligned" was added to the
  issue's list: without it slot_dropped stayed within 6.5x of the bound at K = 4224.
"""
import functools
import math

import pytest
import torch

from tests import skinny_ref as R
from tests.skinny_ref import Structure

ROWS = 4
MARGIN = 10.0
ROW_STRUCTS = ("wave", Structure("lds", 0, 3, 6, 5, 4), Structure("lds", 0, 3, 3, 4, 4))
LOGITS_STRUCTS = (Structure("wave", 4, 0, 0, 0, 1), Structure("lds", 0, 1, 8, 4, 1), Structure("lds", 0, 1, 4, 4, 1))
SILU_STRUCTS = (Structure("lds", 0, 2, 8, 4, 1), Structure("lds", 0, 1, 8, 4, 1), Structure("lds", 0, 1, 8, 2, 1), Structure("lds", 0, 1, 4, 4, 1))
FOLDS = ((False, False), (True, False), (True, True))          # (fold, sum(x^2) left by an SK_ROW epilogue instead of the producer)


def shapes():
    """(mode, structure, K, N, fold, striped)"""
    out = []
    for K in R.K_LIST:
        for st in ROW_STRUCTS:
            st = Structure("wave", 8 if K % 256 == 0 else 4, 0, 0, 0, 1) if st == "wave" else st
            out += [("row", st, K, N, False, False) for N in (64, 320)]
        for st in LOGITS_STRUCTS:
            out += [("logits", st, K, N, f, s) for N in (320, 323) for f, s in FOLDS if N == 323 or f]
        for st in SILU_STRUCTS:
            out += [("silu_mul", st, K, 256, f, s) for f, s in FOLDS]
    return out


def evaluate(shape, mut=()):
    """per case: the emulator's worst error / bound on this shape; "row" also the sum(x^2) stripes against the returned fp16 row"""
    mode, st, K, N, fold, striped = shape
    ratios = {}
    for case in R.CASES[mode]:
        if R.needs_fold(mode, case) and not fold:
            continue
        c = _case(case, mode, K, N)
        ref, bound = _bound(case, mode, K, N, fold, striped)
        e = R.emulate(mode, c["x"], c["w"], st, c["resid"], fold, R.EPS, striped, fill=1000.0, mut=mut)
        r = R.worst_ratio(e["out"], ref, bound)
        if mode == "row":
            S, sb = R.ssq_row_bound(e["out"])
            r = max(r, R.worst_ratio(R.ssq_value(e["ssq"]), S, sb))
        ratios[case] = r
    return ratios


@functools.lru_cache(maxsize=None)
def _case(case, mode, K, N):
    return R.build_case(case, mode, ROWS, K, N, seed=K * 31 + N)


@functools.lru_cache(maxsize=None)
def _bound(case, mode, K, N, fold, striped):
    c = _case(case, mode, K, N)
    return R.derived_bound(mode, c["x"], c["w"], c["resid"], fold, R.EPS, striped)


@functools.lru_cache(maxsize=None)
def survey():
    """(worst unmutated ratio per mode, {mutation: (smallest over shapes of the best case's ratio, that shape, shapes it applied to)})"""
    worst = {}
    margins = {m: (math.inf, None, 0) for m in R.MUTATIONS}
    for shape in shapes():
        mode, st, K, N, fold, striped = shape
        worst[mode] = max(worst.get(mode, 0.0), max(evaluate(shape).values()))
        for m in R.MUTATIONS:
            if R.applies(m, mode, st, K, N, ROWS, fold, striped):
                best = max(evaluate(shape, (m,)).values())
                lo, at, n = margins[m]
                margins[m] = (best, shape, n + 1) if best < lo else (lo, at, n + 1)
    return worst, margins


def test_the_emulator_stays_inside_the_bound():
    worst, _ = survey()
    print("emulator worst error / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {"row", "logits", "silu_mul"}
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutant_leaves_the_bound_on_every_shape_it_applies_to(mutation):
    _, margins = survey()
    lo, at, n = margins[mutation]
    print(f"{mutation}: smallest margin {lo:.3g} x bound at {at}, {n} shapes")
    assert n > 0, "the mutation applies to no shape of the survey"
    assert lo >= MARGIN, (mutation, lo, at)


def test_every_lds_instantiation_has_a_wrapping_and_a_ragged_k():
    """K_LIST against the ring geometry of every instantiation launch_skx_nb can pick.  K % 128 == 0 makes K / 32 a multiple of 4, so a
    single-split structure of 4-tile chunks can never have a ragged last chunk: the one hole no K fills."""
    for st in set(ROW_STRUCTS[1:] + LOGITS_STRUCTS[1:] + SILU_STRUCTS):
        tab = [R.chunk_table(st, K) for K in R.K_LIST]
        assert any(wraps for _, wraps, _ in tab), st
        assert any(ragged for _, _, ragged in tab) or (st.KC == 4 and st.S == 1), st


def test_structure_follows_the_capacity():
    assert R.structure("row", 2, 256, 1) == Structure("wave", 8, 0, 0, 0, 1) and R.structure("row", 2, 1152, 1).NW == 4
    assert R.structure("row", 64, 2304, 4).kind == "wave" and R.structure("row", 64, 2304, 4, row_split_min_k=128) == ROW_STRUCTS[1]
    assert R.structure("row", 128, 128, 1) == ROW_STRUCTS[1] and R.structure("row", 128, 128, 5) == ROW_STRUCTS[2]
    assert R.structure("logits", 2, 128, 1).kind == "wave" and R.structure("logits", 128, 128, 8).KC == 4
    assert [R.structure("silu_mul", mb, 128, nb, half=h) for mb, nb, h in ((2, 1, 0), (64, 4, 0), (128, 2, 0), (128, 8, 0), (128, 8, 1))] == \
        [SILU_STRUCTS[0], SILU_STRUCTS[0], SILU_STRUCTS[1], SILU_STRUCTS[2], SILU_STRUCTS[3]]


def test_large_rows_sit_at_a_quarter_of_the_accumulator_capacity():
    """one conversion saturates at 2^63 units = 2^35, the 64-bit sum of the stripes wraps at 2^36: rows of 2^34 are inside both, whether the
    producer wrote them (one conversion) or an SK_ROW epilogue did (K / 16 of them)"""
    for K in R.K_LIST:
        x = R.build_case("large", "logits", ROWS, K, 320, seed=K)["x"]
        s = (x.double() ** 2).sum(-1)
        assert 0.9 * R.SSQ_LIMIT / 4 <= float(s[0]) <= R.SSQ_LIMIT / 4 * 1.01
        for slots in (R.emu_ssq_producer(x), R.emu_ssq_row(x)):
            assert int(slots.max()) < 2 ** 63 and (slots >= 0).all()
            assert torch.allclose(R.ssq_value(slots), s, rtol=K * R.U32 + 1e-9, atol=2.0 ** -20)
    assert 17 * 65504.0 ** 2 > R.SSQ_LIMIT                 # fp16 rows CAN exceed it; nothing checks for that

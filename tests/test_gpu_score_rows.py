"""GPU: score_rows_kernel alone (aur_score_rows) against the float64 definition in aurora_amd/scoring.py on the same fp32 rows.

Bound on a log-probability: |lp - ref| <= 1e-5 + 1e-6 * |ref|.  Where it comes from: the kernel computes (l_t - m) - log S with two
fp32 roundings on l_t - m and log S (each <= 2^-24 relative, plus <= 2 ulp for logf), S from fp32 expf (<= 2 ulp each) added in fp32.
Element e belongs to thread (e / 4) % 1024, which adds its ceil(V / 4096) * 4 <= 32 elements (V <= 32768) in order; the partial sums
join in a 6-level butterfly inside a wave and a 4-level one across the 16 waves.  So an element passes through at most 32 + 6 + 4 = 42
additions - inside the V / 1024 + 12 = 44 the bound was worked out for - and the relative error of S is below 42 * 2^-24 + 2 ulp =
2.7e-6, which is also its absolute effect on log S.  Together about 3e-6 + 6e-8 * (|l_t - m| + |log S|); the bound leaves 3x over that.
The argmax has no tolerance: the first index of the maximum."""
import numpy as np
import pytest
import torch

from aurora_amd import scoring
from tests.test_gpu_llm import LLM_CFGS, make_engine

pytestmark = pytest.mark.gpu

VOCABS = [320, 323, 9000, 32000]
ROWS = [1, 5, 128]


@pytest.fixture(scope="module")
def eng():
    e, _ = make_engine(LLM_CFGS["hd32"], 3, max_batch=1)
    yield e
    e.close()


def make_rows(V, n, seed):
    """n rows cycling through the row kinds, with a target each: (logits fp32 [n, V], targets)"""
    g = np.random.default_rng(seed)
    lg = np.empty((n, V), np.float32)
    tg = np.empty(n, np.int64)
    for r in range(n):
        kind = r % 6
        row = (g.standard_normal(V) * 4).astype(np.float32)                  # N(0, 4^2)
        t = int(g.integers(0, V))
        if kind == 1:                                                        # eight boosted tokens, as a language model's row
            hot = g.choice(V, 8, replace=False)
            row[hot] += np.float32(12)
            t = int(hot[3])
        elif kind == 2:                                                      # all equal: lp = -log V, a = 0
            row[:] = np.float32(g.standard_normal() * 4)
        elif kind == 3:                                                      # an exact tie at the maximum: the first index wins
            i, j = sorted(g.choice(V, 2, replace=False).tolist())
            row[i] = row[j] = np.float32(row.max() + 1.5)
            t = [i, j][(r // 6) % 2]
        elif kind == 4:                                                      # values near 6e4: exp overflows unless the maximum is subtracted
            row = (6.0e4 + g.standard_normal(V) * 4).astype(np.float32)
        elif kind == 5:
            t = int(row.argmin()) if (r // 6) % 2 else int(row.argmax())            # target = the minimum / the argmax
        lg[r], tg[r] = row, t
    return lg, tg.tolist()


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("n", ROWS)
def test_rows_against_the_float64_definition(eng, V, n):
    lg, tg = make_rows(V, n, 100 * V + n)
    lp, am = eng.score_rows(torch.from_numpy(lg).cuda(), tg)
    ref_lp, ref_am = scoring.score_rows(lg, tg)
    worst = 0.0
    for r in range(n):
        assert am[r] == ref_am[r], (r, r % 6)
        err, bound = abs(float(lp[r]) - ref_lp[r]), 1e-5 + 1e-6 * abs(ref_lp[r])
        worst = max(worst, err / bound)
        assert err <= bound, (r, r % 6, float(lp[r]), ref_lp[r])
    print(f"score_rows V={V} rows={n}: worst error / bound = {worst:.3f}")
    for r in range(2, n, 6):                                                 # all equal
        assert am[r] == 0 and abs(float(lp[r]) + np.log(V)) <= 1e-5 + 1e-6 * np.log(V)
    for r in range(3, n, 6):                                                 # the tie: greedy only for the first of the two
        assert (am[r] == tg[r]) == ((r // 6) % 2 == 0)


@pytest.mark.parametrize("V", VOCABS)
def test_a_row_scores_the_same_bits_wherever_it_lies(eng, V):
    """row index 0 of a one-row call and row index 127 of a 128-row call; with V % 4 != 0 the two rows differ in alignment too"""
    lg, tg = make_rows(V, 128, 7 * V)
    one_lp, one_am = eng.score_rows(torch.from_numpy(lg[5:6].copy()).cuda(), tg[5:6])
    big = lg.copy()
    big[127] = lg[5]
    tgb = list(tg)
    tgb[127] = tg[5]
    lp, am = eng.score_rows(torch.from_numpy(big).cuda(), tgb)
    assert lp[127].tobytes() == one_lp[0].tobytes() == lp[5].tobytes() and am[127] == one_am[0] == am[5]
    # the same rows at an address that is not 16-byte aligned: the element-wise loads add in the same order
    flat = torch.empty(128 * V + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(big).cuda().reshape(-1)
    lp2, am2 = eng.score_rows(flat[1:].view(128, V), tgb)
    assert lp2.tobytes() == lp.tobytes() and am2.tobytes() == am.tobytes()


@pytest.mark.parametrize("V", [320, 323])
def test_unused_targets(eng, V):
    lg, tg = make_rows(V, 5, 11)
    tg[1], tg[3] = -1, V
    dev = torch.from_numpy(lg).cuda()
    dev[1] = float("nan")                                                   # not read
    lp, am = eng.score_rows(dev, tg)
    assert am[1] == am[3] == -1 and lp[1] == lp[3] == 0.0
    ref_lp, ref_am = scoring.score_rows(lg, tg)
    for r in (0, 2, 4):
        assert am[r] == ref_am[r] and abs(float(lp[r]) - ref_lp[r]) <= 1e-5 + 1e-6 * abs(ref_lp[r])

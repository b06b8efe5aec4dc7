"""GPU: token_logprob_rows_kernel alone (aur_token_logprob_rows) - the evaluation the decode path runs behind every pick - against
aur_score_rows (bitwise) and against the float64 definition in aurora_amd/scoring.py on the same fp32 rows.

Bound on every log-probability, the picked token's and each alternative's: |lp - ref| <= 1e-5 + 1e-6 * |ref|, the bound
tests/test_gpu_score_rows.py derives for (l_t - m) - log S.  An alternative goes through the same arithmetic: its value v takes the
place of l_t, m and log S are the same numbers.  The ids have no tolerance: the order (value descending, index ascending) is exact in
fp32 as in float64, because the conversion of the rows is."""
import numpy as np
import pytest
import torch

from aurora_amd import scoring
from tests.test_gpu_llm import LLM_CFGS, make_engine
from tests.test_gpu_score_rows import make_rows

pytestmark = pytest.mark.gpu

VOCABS = [5, 320, 323, 9000, 32000]       # below top_n, aligned, unaligned rows, uneven quads per thread, several quads per thread
ROWS = [1, 5, 128]
TOPS = [0, 1, 8]


@pytest.fixture(scope="module")
def eng():
    e, _ = make_engine(LLM_CFGS["hd32"], 3, max_batch=1)
    yield e
    e.close()


def rows_of(V, n, seed):
    """`make_rows` of tests/test_gpu_score_rows.py.  It boosts 8 distinct tokens in every sixth row, which a vocabulary of 5 does not
    have: there the same row kinds are drawn here, with every token of the row boosted in that kind."""
    if V >= 8:
        return make_rows(V, n, seed)
    g = np.random.default_rng(seed)
    lg = np.empty((n, V), np.float32)
    tg = []
    for r in range(n):
        kind = r % 6
        row = (g.standard_normal(V) * 4).astype(np.float32)
        t = int(g.integers(0, V))
        if kind == 1:
            row += np.float32(12)
        elif kind == 2:
            row[:] = np.float32(g.standard_normal() * 4)
        elif kind == 3:
            i, j = sorted(g.choice(V, 2, replace=False).tolist())
            row[i] = row[j] = np.float32(row.max() + 1.5)
            t = [i, j][(r // 6) % 2]
        elif kind == 4:
            row = (6.0e4 + g.standard_normal(V) * 4).astype(np.float32)
        elif kind == 5:
            t = int(row.argmin()) if (r // 6) % 2 else int(row.argmax())
        lg[r] = row
        tg.append(t)
    return lg, tg


_REF = {}


def reference(V, n):
    """rows, tokens and the float64 definition at top_n = 8, computed once per shape (the first k ranks of 8 are the k ranks)"""
    if (V, n) not in _REF:
        lg, tg = rows_of(V, n, 100 * V + n)
        _REF[V, n] = (lg, tg) + scoring.token_logprob_rows(lg, tg, 8)
    return _REF[V, n]


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("n", ROWS)
def test_rows_against_score_rows_and_the_float64_definition(eng, V, n):
    lg, tg, ref_lp, ref_ids, ref_lps = reference(V, n)
    dev = torch.from_numpy(lg).cuda()
    score_lp, score_am = eng.score_rows(dev, tg)
    worst = 0.0
    for top in TOPS:
        lp, ids, lps = eng.token_logprob_rows(dev, tg, top)
        assert lp.dtype == np.float32 and ids.shape == lps.shape == (n, top)
        assert lp.tobytes() == score_lp.tobytes(), ("not the bits of aur_score_rows", top)
        assert np.array_equal(ids, ref_ids[:, :top]), top                        # ties included
        if top:
            assert np.array_equal(ids[:, 0], score_am)                           # rank 0 = score_rows' first argmax
        for r in range(n):
            pairs = [(float(lp[r]), ref_lp[r])] + [(float(lps[r, k]), ref_lps[r, k]) for k in range(top)]
            for got, ref in pairs:
                err, bound = abs(got - ref), 1e-5 + 1e-6 * abs(ref)
                worst = max(worst, err / bound)
                assert err <= bound, (top, r, r % 6, got, ref)
            for k in range(min(top, V), top):                                     # ranks at or beyond the vocabulary
                assert ids[r, k] == -1 and lps[r, k] == 0.0
        for r in range(2, n, 6):                                                  # all equal: ids 0 .. top-1
            assert ids[r].tolist() == [k if k < V else -1 for k in range(top)]
        for r in range(3, n, 6):                                                  # the tie at the maximum: lower index first, same lp bits
            if top == 8:
                assert ids[r, 0] < ids[r, 1] and lps[r, 0].tobytes() == lps[r, 1].tobytes()
    print(f"token_logprob_rows V={V} rows={n}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("V", VOCABS)
def test_a_row_gives_the_same_bits_wherever_it_lies(eng, V):
    """row index 0 of a one-row call, row index 127 of a 128-row call, and a base address that is not 16-byte aligned"""
    lg, tg = rows_of(V, 128, 7 * V)
    one = eng.token_logprob_rows(torch.from_numpy(lg[5:6].copy()).cuda(), tg[5:6], 8)
    big = lg.copy()
    big[127] = lg[5]
    tgb = list(tg)
    tgb[127] = tg[5]
    full = eng.token_logprob_rows(torch.from_numpy(big).cuda(), tgb, 8)
    for a, b in zip(one, full):
        assert a[0].tobytes() == b[127].tobytes() == b[5].tobytes()
    flat = torch.empty(128 * V + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(big).cuda().reshape(-1)
    off = eng.token_logprob_rows(flat[1:].view(128, V), tgb, 8)
    for a, b in zip(off, full):
        assert a.tobytes() == b.tobytes()
    lp, _ = eng.score_rows(flat[1:].view(128, V), tgb)
    assert lp.tobytes() == full[0].tobytes()


@pytest.mark.parametrize("V", [5, 320, 323])
def test_unused_tokens_leave_the_row_unread(eng, V):
    lg, tg = rows_of(V, 5, 11)
    tg[1], tg[3] = -1, V
    dev = torch.from_numpy(lg).cuda()
    dev[1] = float("nan")                                                         # not read
    for top in TOPS:
        lp, ids, lps = eng.token_logprob_rows(dev, tg, top)
        for r in (1, 3):
            assert lp[r] == 0.0 and (ids[r] == -1).all() and (lps[r] == 0.0).all()
        ref_lp, ref_ids, ref_lps = scoring.token_logprob_rows(lg, tg, top)
        for r in (0, 2, 4):
            assert np.array_equal(ids[r], ref_ids[r]) and abs(float(lp[r]) - ref_lp[r]) <= 1e-5 + 1e-6 * abs(ref_lp[r])


def test_a_row_without_a_maximum_and_bad_arguments(eng):
    """all NaN: score_rows' token 0 at rank 0, nothing behind it; top_n outside [0, 8] is refused before any launch"""
    dev = torch.full((2, 323), float("nan"), device="cuda")
    dev[1] = torch.arange(323, device="cuda").float()
    lp, ids, lps = eng.token_logprob_rows(dev, [4, 4], 3)
    s_lp, s_am = eng.score_rows(dev, [4, 4])
    assert s_am[0] == 0 and ids[0].tolist() == [0, -1, -1] and np.isnan(lp[0]) and np.isnan(lps[0, 0]) and lps[0, 1:].tolist() == [0.0, 0.0]
    assert ids[1].tolist() == [322, 321, 320] and lp[1].tobytes() == s_lp[1].tobytes()
    with pytest.raises(ValueError):
        eng.token_logprob_rows(dev, [4, 4], 9)
    assert eng.L.aur_logprob_bytes(eng.ctx, 9) == -1 and eng.L.aur_logprob_bytes(eng.ctx, 0) > 0

"""CPU: the definition of a generated token's log-probability and its top-n alternatives (aurora_amd/scoring.py token_logprobs) against
torch.log_softmax + torch.topk in float64, its agreement with `score_rows`, its tie / short-row / unused-token rules, and the host
checks of the `logprobs=` argument, which come before any GPU call."""
import numpy as np
import pytest
import torch

from aurora_amd import scoring


def rows(V, n, seed):
    g = np.random.default_rng(seed)
    lg = np.empty((n, V), np.float32)
    for r in range(n):                                                # N(0, 4^2) in fp32 without ties: distinct values of a larger draw
        u = np.unique((g.standard_normal(2 * V + 8) * 4).astype(np.float32))
        lg[r] = g.permutation(u)[:V]
        assert len(np.unique(lg[r])) == V
    return lg, g.integers(0, V, n).tolist()


@pytest.mark.parametrize("V", [5, 323, 32000])
def test_definition_against_log_softmax_and_topk(V):
    lg, tok = rows(V, 4, V)
    for n in (0, 1, 8):
        lp, ids, lps = scoring.token_logprob_rows(lg, tok, n)
        assert lp.dtype == np.float64 and ids.shape == lps.shape == (4, n) and ids.dtype == np.int32
        ref = torch.log_softmax(torch.from_numpy(lg).double(), -1)
        k = min(n, V)
        top = torch.topk(ref, k, -1) if k else None
        for r in range(4):
            # float64 on both sides; the two differ in the order of the additions of V terms only
            assert abs(lp[r] - ref[r, tok[r]].item()) <= 1e-12 * max(1.0, abs(lp[r]))
            if k:
                assert ids[r, :k].tolist() == top.indices[r].tolist()
                np.testing.assert_allclose(lps[r, :k], top.values[r].numpy(), rtol=0, atol=1e-11)
            assert (ids[r, k:] == -1).all() and (lps[r, k:] == 0).all()


def test_token_logprob_is_score_rows_value_and_rank_0_its_argmax():
    lg, tok = rows(323, 6, 9)
    lg[2] = lg[2, 0]                                                  # an all-equal row
    lg[3, 7] = lg[3, 200] = lg[3].max() + 1                           # a tie at the maximum
    want_lp, want_am = scoring.score_rows(lg, tok)
    for r in range(6):
        lp, ids, lps = scoring.token_logprobs(lg[r], tok[r], 3)
        assert lp == want_lp[r] == scoring.token_logprobs(lg[r], tok[r])[0]
        assert ids[0] == want_am[r]
        l = lg[r].astype(np.float64)
        assert lps[0] == -np.log(np.sum(np.exp(l - l[ids[0]])))       # rank 0: lp = -log S


def test_tie_order_all_equal_rows_short_rows_and_unused_tokens():
    row = np.array([1.0, 3.0, 2.0, 3.0, 2.0, 3.0, -1.0], np.float32)
    lp, ids, lps = scoring.token_logprobs(row, 3, 8)
    assert ids.tolist() == [1, 3, 5, 2, 4, 0, 6, -1]                  # value descending, index ascending; rank 7 >= V
    assert lps[7] == 0.0 and lps[0] == lps[1] == lps[2] and lps[3] == lps[4] and lp == lps[1]
    assert (np.diff(lps[:7]) <= 0).all()
    eq = np.full(40, np.float32(-2.5))
    lp, ids, lps = scoring.token_logprobs(eq, 17, 8)
    assert ids.tolist() == list(range(8)) and np.allclose(lps, -np.log(40.0), rtol=0, atol=1e-15) and abs(lp + np.log(40.0)) <= 1e-15
    lp, ids, lps = scoring.token_logprobs(np.array([0.5, 1.5, -1.0], np.float32), 0, 5)         # V < n
    assert ids.tolist() == [1, 0, 2, -1, -1] and lps[3:].tolist() == [0.0, 0.0] and lp == lps[1]
    for t in (-1, 3, 1 << 20):                                        # outside [0, V): unused, score_rows' convention
        lp, ids, lps = scoring.token_logprobs(np.array([0.5, 1.5, np.nan], np.float32), t, 4)
        assert lp == 0.0 and ids.tolist() == [-1] * 4 and lps.tolist() == [0.0] * 4
    assert scoring.score_rows(np.zeros((1, 3), np.float32), [3])[0][0] == 0.0
    lp, ids, lps = scoring.token_logprobs(np.full(6, np.nan, np.float32), 2, 3)                 # no maximum: score_row's token 0 alone
    assert np.isnan(lp) and ids.tolist() == [0, -1, -1] and np.isnan(lps[0]) and lps[1:].tolist() == [0.0, 0.0]
    assert scoring.score_row(np.full(6, np.nan, np.float32), 2)[1] == 0


@pytest.mark.parametrize("bad", [-1, 9, 2.0, "2", True])
def test_logprobs_range_check_comes_before_any_gpu_call(bad):
    """An engine object that was never constructed has no ctx, no library and no device: reaching for any of them raises
    AttributeError, so a ValueError shows that the check ran first."""
    from aurora_amd.engine import AuroraCapEngine
    from aurora_amd.model import AuroraModel, _LLM
    with pytest.raises(ValueError):
        scoring.check_logprobs(bad)
    eng = AuroraCapEngine.__new__(AuroraCapEngine)
    px = torch.zeros(1, 3, 56, 56)
    for call in (lambda: eng.generate([None], [4], 4, logprobs=bad),
                 lambda: eng.caption_ids(px, [1, -200], 0.5, 4, logprobs=bad),
                 lambda: eng.caption_batch([(px, [1, -200])], 0.5, 4, logprobs=bad),
                 lambda: eng.caption_prompts(px, [[1, -200]], 0.5, 4, logprobs=bad),
                 lambda: next(eng.caption_stream([(px, [1, -200])], 0.5, 4, logprobs=bad)),
                 lambda: eng.token_logprob_rows(None, [0], bad)):
        with pytest.raises(ValueError):
            call()
    llm = _LLM.__new__(_LLM)
    with pytest.raises(ValueError):
        llm.generate(inputs_embeds=torch.zeros(1, 4, 8), return_dict_in_generate=True, output_logprobs=True, top_logprobs=bad)
    with pytest.raises(ValueError):
        llm.generate(inputs_embeds=torch.zeros(1, 4, 8), output_logprobs=True)          # needs return_dict_in_generate=True
    m = AuroraModel.__new__(AuroraModel)
    with pytest.raises(ValueError):
        m.caption_batch([(px, [1, -200])], logprobs=bad)
    assert scoring.check_logprobs(None) is None and scoring.check_logprobs(0) == 0 and scoring.check_logprobs(np.int64(8)) == 8


def test_abi_declares_and_binds_the_logprob_entry_points():
    """tests/test_lib_abi.py holds the header and the binding to each other as a whole; these are the names this feature adds"""
    from aurora_amd import _lib
    from tests.test_lib_abi import header_symbols
    new = {"aur_logprob_bytes", "aur_logprob_enable", "aur_get_logprobs", "aur_slot_collect_logprobs", "aur_token_logprob_rows"}
    assert new <= set(header_symbols()) and new <= set(_lib.SIGNATURES)
    assert set(header_symbols()) == set(_lib.SIGNATURES)

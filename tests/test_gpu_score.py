"""GPU: `aur_llm_score_var` - any rows of a prefill pass through the pick path's lm_head and score_rows_kernel.

The yardstick is the existing single-sequence path in the same process.  CONTRACT: an entry naming row r of sequence i has BITWISE the
logits row `logits()` returns after `prefill(slot, embeds_i[: pos0 + r + 1], pos0 + r + 1)`, that prefill's greedy first token as its
argmax, and the log-probability `score_rows` gives on that row.  Everything here is bitwise except the comparison with the CPU oracle.

No test passes an out-of-range value in DEVICE memory other than the documented -1 holes."""
import numpy as np
import pytest
import torch

from aurora_amd import scoring
from oracle import aurora_oracle as O
from tests.parity_bounds import LOGIT_TOL
from tests.test_gpu_llm import LLM_CFGS, make_engine, padded
from tests.test_gpu_prefill_var import NAN16, rand_embeds, strided
from tests.util import rand_llm_weights

pytestmark = pytest.mark.gpu

NAMES = ["hd32", "hd128"]


def targets_for(cfg, n, seed):
    return np.random.default_rng(seed).integers(0, cfg["vocab_size"], size=n).astype(np.int32).tolist()


def contract(eng, emb, positions):
    """[(logits row, greedy first token)] of prefill(slot 0, emb[: p + 1]) for every position p: the existing path"""
    out = []
    for p in positions:
        eng.begin_batch(1, 1, None)
        eng.prefill(0, padded(emb[:p + 1].float()), p + 1)
        out.append((eng.logits()[0].clone(), eng.outputs()[0][0]))
    return out


def score(eng, embs, stride, rows, targets, pos0=0, seq0=0, fill=NAN16, batch=None):
    """one eager call over `embs` (the rows of the pass), padding rows filled with `fill` -> (logprob, argmax, logits) on the host side"""
    if batch is not None:
        eng.begin_batch(batch, 1, None)
    lp, am, lg = eng.score_stage(seq0, len(embs), strided(embs, stride, fill), pos0, stride, [e.shape[0] for e in embs], rows, targets,
                                 want_logits=True)
    torch.cuda.synchronize()
    return lp.clone(), am.clone(), lg.clone()


def assert_entries_equal(got, want, live):
    for j in live:
        assert got[0][j].cpu().numpy().tobytes() == want[0][j].cpu().numpy().tobytes(), j
        assert int(got[1][j]) == int(want[1][j]), j
        assert torch.equal(got[2][j], want[2][j]), j


@pytest.mark.parametrize("name", NAMES)
def test_a_contract_rows_across_a_page_boundary(name):
    """(a) context 60, continuation 9: rows 59 .. 67 cross the 64-token page; stride 96; max_batch 2, so five lm_head chunks"""
    cfg = LLM_CFGS[name]
    emb = rand_embeds(cfg, [68], 80)[0]
    rows, tg = list(range(59, 68)), targets_for(cfg, 9, 1)
    eng, _ = make_engine(cfg, 41, max_batch=2, max_ctx=576, max_new=16)
    try:
        lp, am, lg = score(eng, [emb], 96, rows, tg, batch=1)
        for j, (want_lg, want_tok) in enumerate(contract(eng, emb, rows)):
            assert torch.equal(lg[j], want_lg), j
            assert int(am[j]) == want_tok == int(torch.argmax(want_lg)), j
        klp, kam = eng.score_rows(lg, tg)
        assert klp.tobytes() == lp.cpu().numpy().tobytes() and kam.tolist() == am.cpu().tolist()
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_b_against_the_oracle(name):
    """(b) teacher-forced oracle logits -> scoring.score_row in float64.  Log-sum-exp and the target logit are each 1-Lipschitz in the
    sup norm, the logits are within LOGIT_TOL * max|logit| of the oracle's: |dlp| <= 2 * LOGIT_TOL * max|logit| per token; the argmax
    equals the oracle's wherever its top-2 margin exceeds the same (the suite's margin rule)."""
    cfg = LLM_CFGS[name]
    emb = rand_embeds(cfg, [68], 81)[0]
    rows = list(range(59, 68))
    eng, w = make_engine(cfg, 42, max_batch=2, max_ctx=576, max_new=16)
    try:
        h, _ = O.llama_forward(emb.float(), w, cfg, None, 0)
        ref = torch.nn.functional.linear(h[rows], w["lm_head.weight"])
        tg = [int(ref[j].argmax()) if j % 2 else t for j, t in enumerate(targets_for(cfg, 9, 2))]      # likely and unlikely targets
        lp, am, _ = score(eng, [emb], 96, rows, tg, batch=1)
        scale = ref.abs().max().item()
        checked = 0
        for j in range(9):
            rlp, ra = scoring.score_row(ref[j].numpy(), tg[j])
            err = abs(float(lp[j]) - rlp)
            print(f"score vs oracle [{name}] token {j}: |dlp| = {err:.3e}, bound {2 * LOGIT_TOL * scale:.3e}")
            assert err <= 2 * LOGIT_TOL * scale, (j, float(lp[j]), rlp)
            top2 = ref[j].topk(2).values
            if (top2[0] - top2[1]).item() > 2 * LOGIT_TOL * scale:
                assert int(am[j]) == ra, j
                checked += 1
        assert checked >= 1
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_c_four_sequences_holes_and_chunks(name):
    """(c) lengths [33, 96, 70, 65] in one pass, NaN in the padding rows, -1 holes in the entry arrays: each sequence as alone.  Then 11
    entries on a max_batch = 2 engine - six lm_head chunks - against the same entries scored one per call (two sequences there: a pass
    holds at most max_batch sequences, like every _var call)."""
    cfg, lens, stride = LLM_CFGS[name], [33, 96, 70, 65], 96
    embs = rand_embeds(cfg, lens, 82)
    pos = [[0, 31, 32], [63, 64, 95], [5, 69], [64]]                        # scored positions per sequence
    rows, live = [], []
    for i, ps in enumerate(pos):
        rows.append(-1)
        for p in ps:
            live.append(len(rows))
            rows.append(i * stride + p)
    rows.append(-1)
    tg = targets_for(cfg, len(rows), 3)
    eng, _ = make_engine(cfg, 43, max_batch=4, max_ctx=576, max_new=16)
    try:
        got = score(eng, embs, stride, rows, tg, batch=4)
        for j in set(range(len(rows))) - set(live):
            assert int(got[1][j]) == -1 and float(got[0][j]) == 0.0
        j = 0
        for i, ps in enumerate(pos):
            alone = score(eng, [embs[i]], stride, ps, [tg[live[j + k]] for k in range(len(ps))])
            assert_entries_equal([x[[live[j + k] for k in range(len(ps))]] for x in got], alone, range(len(ps)))
            j += len(ps)
    finally:
        eng.close()
    eng, _ = make_engine(cfg, 43, max_batch=2, max_ctx=576, max_new=16)
    try:
        two, rows2 = [embs[1], embs[2]], [0, -1, 95, 96 + 69, 40, -1, 96 + 1, 63, 64, 96 + 33, 7]
        tg2 = targets_for(cfg, 11, 4)
        got = score(eng, two, stride, rows2, tg2, batch=2)
        for j, r in enumerate(rows2):
            if r < 0:
                assert int(got[1][j]) == -1 and float(got[0][j]) == 0.0
            else:
                assert_entries_equal([x[j:j + 1] for x in got], score(eng, two, stride, [r], [tg2[j]]), [0])
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pos0", [64, 192])
def test_d_behind_a_staged_prefix(name, pos0):
    """(d) the prefix staged by `prefill_stage`, the rest through the call at pos0: the pos0 = 0 call over the whole sequence"""
    cfg, new = LLM_CFGS[name], 70
    emb = rand_embeds(cfg, [pos0 + new], 83)[0]
    ps = [0, 5, 63, 64, 69]                                                 # rows of the pass: positions pos0 + p
    tg = targets_for(cfg, len(ps), 5)
    eng, _ = make_engine(cfg, 44, max_batch=2, max_ctx=576, max_new=16)
    try:
        whole = score(eng, [emb], (pos0 + new + 31) // 32 * 32, [pos0 + p for p in ps], tg, batch=1)
        eng.begin_batch(1, 1, None)
        eng.prefill_stage(0, 1, padded(emb[:pos0].float()), pos0)
        assert_entries_equal(score(eng, [emb[pos0:]], 96, ps, tg, pos0=pos0), whole, range(len(ps)))
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_e_the_last_layer_runs_unpruned(name):
    """(e) stride 320, from which hd32 / hd128 prune the last layer of a prefill: `prefill_prune_last` 1 and 0 give the same bits, and a
    scored row in FRONT of the last 128 rows (which a pruned last layer leaves one layer short) equals the contract's prefill."""
    cfg, L, stride = LLM_CFGS[name], 300, 320
    assert stride > 128 and 128 * (3 * cfg["hidden_size"] + cfg["intermediate_size"]) <= stride * cfg["intermediate_size"]
    emb = rand_embeds(cfg, [L], 84)[0]
    ps = [10, 100, 191, 192, 299]
    tg = targets_for(cfg, len(ps), 6)
    eng, _ = make_engine(cfg, 45, max_batch=2, max_ctx=576, max_new=16)
    try:
        on = score(eng, [emb], stride, ps, tg, batch=1)
        eng.set_option("prefill_prune_last", 0)
        off = score(eng, [emb], stride, ps, tg)
        eng.set_option("prefill_prune_last", 1)
        assert_entries_equal(on, off, range(len(ps)))
        for j, (want_lg, want_tok) in zip((1, 4), contract(eng, emb, [100, 299])):
            assert torch.equal(on[2][j], want_lg) and int(on[1][j]) == want_tok, j
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_f_recorded_and_replayed(name):
    """(f) captured once with `graph_capture`, replayed twice with refilled embeds, lengths and entry arrays: each replay is the eager call"""
    cfg, stride, cap = LLM_CFGS[name], 96, 7
    eng, _ = make_engine(cfg, 46, max_batch=2, max_ctx=576, max_new=16)
    try:
        V, d = cfg["vocab_size"], cfg["hidden_size"]
        dev = dict(device="cuda")
        buf = torch.zeros(2 * stride, d, dtype=torch.float16, **dev)
        lens_t, rows_t, tg_t = (torch.zeros(n, dtype=torch.int32, **dev) for n in (2, cap, cap))
        lp, am, lg = torch.zeros(cap, **dev), torch.zeros(cap, dtype=torch.int32, **dev), torch.zeros(cap, V, **dev)
        cases = [([68, 33], [59, 67, -1, 96 + 32, 0, -1, 96 + 1]), ([40, 96], [39, -1, 96 + 95, 96 + 64, 1, 38, -1]), ([96, 65], [95, 96 + 64, 63, 64, -1, -1, 96])]
        eager = []
        for k, (lens, rows) in enumerate(cases):                            # the eager calls first: they also allocate the scratch
            eager.append(score(eng, rand_embeds(cfg, lens, 90 + k), stride, rows, targets_for(cfg, cap, 10 + k), batch=2))
        eng.begin_batch(2, 1, None)
        gid, nodes = eng.graph_capture(lambda: eng.score_stage(0, 2, buf, 0, stride, lens_t, rows_t, tg_t, nscore=cap, logprob_out=lp,
                                                               argmax_out=am, logits_out=lg))
        assert nodes > 0
        for k, (lens, rows) in enumerate(cases[1:], 1):
            buf.copy_(strided(rand_embeds(cfg, lens, 90 + k), stride, NAN16))
            lens_t.copy_(torch.tensor(lens, dtype=torch.int32))
            rows_t.copy_(torch.tensor(rows, dtype=torch.int32))
            tg_t.copy_(torch.tensor(targets_for(cfg, cap, 10 + k), dtype=torch.int32))
            eng.graph_launch(gid)
            torch.cuda.synchronize()
            live = [j for j, r in enumerate(rows) if r >= 0]
            assert_entries_equal((lp, am, lg), eager[k], live)
            assert am.cpu().tolist() == eager[k][1].cpu().tolist() and lp.cpu().numpy().tobytes() == eager[k][0].cpu().numpy().tobytes()
        eng.graph_destroy(gid)
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_g_between_two_decode_calls_on_spare_sequences(name):
    """(g) two slots mid-decode on an engine with two spare KV sequences; a score call on the spare sequences between two `decode`
    calls leaves the decode exactly as an undisturbed run, and is itself what it is on a quiet engine"""
    from aurora_amd.engine import AuroraCapEngine
    cfg = LLM_CFGS[name]
    eng = AuroraCapEngine({"vit": None, "llm": cfg}, {"llm": rand_llm_weights(cfg, 47)}, max_frames=1, max_batch=2, max_ctx=576, max_new_tokens=16,
                          spare_slots=2)
    try:
        prompts = rand_embeds(cfg, [50, 97], 85)
        scored = rand_embeds(cfg, [68, 40], 86)
        rows, tg = [59, 67, 96 + 39, 96 + 0, 64], targets_for(cfg, 5, 7)

        def run(disturb):
            eng.begin_batch(2, 13, None)
            for b, e in enumerate(prompts):
                eng.prefill(b, padded(e.float()), e.shape[0])
            eng.decode(5)
            got = score(eng, scored, 96, rows, tg, seq0=2) if disturb else None
            eng.decode(7)
            return eng.logits().clone(), eng.outputs(), got
        quiet = score(eng, scored, 96, rows, tg, batch=2)
        a, b = run(False), run(True)
        assert a[1] == b[1] and torch.equal(a[0], b[0])
        assert_entries_equal(b[2], quiet, range(5))
    finally:
        eng.close()

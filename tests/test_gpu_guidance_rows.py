"""Classifier-free guidance on the GPU, the kernels alone (aur_guidance_rows): guidance_apply_kernel against the
float64 definition within the bound tests/guidance_ref.py derives, what it must leave untouched bit for bit, and
guidance_restore_kernel.  Vocabulary 32000 takes the 16-byte path, 1003 the scalar one (rows off the 16-byte grid)."""
import functools

import numpy as np
import pytest
import torch

from aurora_amd import guidance as GD
from tests import guidance_ref as R
from tests.test_gpu_llm import LLM_CFGS, make_engine
from tests.util import observe

pytestmark = pytest.mark.gpu
SAVE_FILL = 0x7fc0beef                                       # what guidance_rows fills the save buffer with


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    e, _ = make_engine(LLM_CFGS["hd32"], 5, max_batch=2, max_new=8)
    yield e
    e.close()


# (rows of the buffer, [(leader, partner)], launched range or None): partners below and above their leaders, across the 16-row fragment
# boundary, neutral rows in between, ranges that leave rows out on either side
LAYOUTS = [
    (1, [], None),                                            # one neutral row
    (3, [(0, 2)], None),                                      # a neutral row between the two
    (3, [(2, 1)], (1, 2)),                                    # row 0 outside the launch
    (16, [(5, 0), (7, 12), (15, 14)], None),
    (17, [(16, 15), (3, 9)], None),                           # across the fragment boundary, partner below
    (17, [(15, 16)], (2, 15)),                                # ... partner above; rows 0 and 1 outside
    (32, [(5, 0), (16, 15), (17, 31), (30, 18), (8, 24)], None),
    (32, [(20, 19), (21, 27)], (16, 12)),                     # rows [16, 28) launched: 16 rows before and 4 behind stay out
]


@functools.lru_cache(maxsize=None)
def buffer(V: int, rows: int):
    """rows fp32 [rows, V]: pairs as a model gives them; row 1 (when there is one) repeats row 0, the last row has a spread of 200"""
    rng = np.random.default_rng(V + rows)
    out = np.stack([x for _ in range((rows + 1) // 2) for x in R.row_pair(rng, V)])[:rows].copy()
    if rows > 1:
        out[1] = out[0]
    if rows > 2:
        w = out[-1]
        out[-1] = (w * np.float32(200.0 / (w.max() - w.min()))).astype(np.float32)
    out.setflags(write=False)
    return out


def run(eng, V, rows, pairs, rng_, g, restore=False):
    buf = buffer(V, rows)
    recs = GD.records(g, pairs, rows)
    b0, nb = rng_ if rng_ is not None else (0, rows)
    got, save = eng.guidance_rows(torch.from_numpy(buf.copy()).cuda(), recs, restore=restore, b0=b0, nb=nb)
    return buf, recs, got.cpu().numpy(), save.cpu().numpy()


@pytest.mark.parametrize("V", [32000, 1003])
@pytest.mark.parametrize("g", R.SCALES)
def test_apply_is_the_definition_within_the_derived_bound_and_touches_nothing_else(eng, V, g):
    guided = 0
    for rows, pairs, rng_ in LAYOUTS:
        buf, recs, got, save = run(eng, V, rows, pairs, rng_, g)
        leaders = {l: p for l, p in pairs}
        for b in range(rows):
            if b in leaders:
                want = GD.apply(buf[b], buf[leaders[b]], g)
                assert np.isfinite(got[b]).all()
                ratio = float(np.abs(got[b].astype(np.float64) - want).max()) / R.bound(buf[b], buf[leaders[b]], g)
                observe(f"guidance/rows_error_over_derived_bound[v{V}]", ratio, 1.0)
                assert np.array_equal(bits(save[b]), bits(buf[b])), (rows, b)           # the leader's original, bitwise
                guided += 1
            else:                                                                        # neutral rows, partners, rows outside the launch
                assert np.array_equal(bits(got[b]), bits(buf[b])), (rows, b)
                assert (save[b].view(np.uint32) == SAVE_FILL).all(), (rows, b)
    assert guided == sum(len(p) for _, p, _ in LAYOUTS)


def test_a_pair_of_identical_rows_gives_the_rows_log_softmax(eng):
    """c == u: lc - lu is exactly 0 whatever the scale, so out is lu bit for bit - and that is score_rows' log-probability of every token"""
    for V in (32000, 1003):
        buf = buffer(V, 3)
        assert np.array_equal(buf[0], buf[1])
        outs = []
        for g in R.SCALES:
            recs = GD.records(g, [(0, 1)], 3)
            got, _ = eng.guidance_rows(torch.from_numpy(buf.copy()).cuda(), recs)
            outs.append(got[0].cpu().numpy())
        assert all(np.array_equal(bits(o), bits(outs[0])) for o in outs)
        toks = [0, 1, V // 2, V - 1, int(np.argmax(buf[0]))]
        rows = torch.from_numpy(np.stack([buf[0]] * len(toks))).cuda()
        lp, _ = eng.score_rows(rows, toks)
        assert np.array_equal(bits(outs[0][toks]), bits(lp))


@pytest.mark.parametrize("V", [32000, 1003])
def test_restore_gives_the_whole_buffer_back_and_two_launches_agree(eng, V):
    for rows, pairs, rng_ in LAYOUTS:
        buf, _, back, _ = run(eng, V, rows, pairs, rng_, 3.0, restore=True)
        assert np.array_equal(bits(back), bits(buf)), rows
        _, _, a, sa = run(eng, V, rows, pairs, rng_, 3.0)
        _, _, b, sb = run(eng, V, rows, pairs, rng_, 3.0)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), rows


def test_records_the_host_would_reject_are_neutral_and_a_wild_partner_is_clamped(eng):
    V = 1003
    buf = buffer(V, 3)
    recs = np.zeros(3, GD.RECORD)
    for bad in (0.0, -2.0, 1.0, np.nan, np.inf):
        recs["scale"], recs["partner"] = [bad, 0, 0], [2, 0, 0]
        got, save = eng.guidance_rows(torch.from_numpy(buf.copy()).cuda(), recs)
        assert np.array_equal(bits(got.cpu().numpy()), bits(buf)) and (save.cpu().numpy().view(np.uint32) == SAVE_FILL).all()
    # a partner index outside the buffer is clamped into it before it addresses anything: 10 ** 6 -> the last row, -5 -> row 0
    for wild, row in ((10 ** 6, 2), (-5, 0)):
        rec_d = np.zeros(3, GD.RECORD)
        rec_d[1] = (1.5, wild)
        out = torch.from_numpy(buf.copy()).cuda()
        save = torch.zeros_like(out)
        from aurora_amd._lib import check
        rec_t = torch.from_numpy(rec_d.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        check(eng.ctx, eng.L.aur_guidance_rows(eng.ctx, out.data_ptr(), 3, V, rec_t.data_ptr(), save.data_ptr(), 0, eng._stream()),
              "aur_guidance_rows")
        torch.cuda.synchronize()
        want = GD.apply(buf[1], buf[row], 1.5)
        assert float(np.abs(out[1].cpu().numpy().astype(np.float64) - want).max()) <= R.bound(buf[1], buf[row], 1.5)

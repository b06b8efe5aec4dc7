"""One decode projection alone - launch_skinny in its SK_ROW, SK_SILU_MUL and SK_LOGITS epilogues, with and without the folded RMSNorm,
behind the production producer of x fragments - against the fp64 definition, elementwise, under the bound derived from the kernels'
stated arithmetic (tests/skinny_ref.py; nothing here is an observed tolerance).  The launches are reached through aur_decode_proj_rows,
which picks the structure exactly as the decode step of an engine of that capacity does.  tests/test_skinny_reference.py shows on the
CPU that each of twelve ways these epilogues can be wrong leaves this bound by more than 10x at every shape it applies to.

Structure by capacity (tests/skinny_ref.py structure; K / 32 tiles, S k splits, KC tiles per chunk, ring of NBUF chunks):

    capacity   SK_ROW                                   SK_LOGITS                 SK_SILU_MUL
    2          per wave, 8 waves (K % 256 == 0) or 4    per wave, 4 waves         LDS, 2 k phases, KC 8, NBUF 4
    64         per wave; "skinny_row_split_min_k" 128:  LDS, KC 8, NBUF 4         LDS, 2 k phases, KC 8, NBUF 4
               LDS split-K S 4, 3 k phases, KC 6, NBUF 5
    128        LDS split-K S 4: KC 6, NBUF 5 up to 4    LDS, KC 8 (KC 4 from 5    LDS, 1 k phase: KC 8, NBUF 4 up to 4 groups; from 5
               column groups, KC 3, NBUF 4 from 5       column groups), NBUF 4    groups KC 8, NBUF 2 (full grid) or KC 4, NBUF 4 (half)

Chunks per split at K = 128, 256, 1152, 2304, 4224 (K / 32 = 4, 8, 36, 72, 132) - w: the ring wraps, r: the last chunk is ragged:

    S 1, KC 8, NBUF 4:   1 r    1      5 w r   9 w     17 w r
    S 1, KC 8, NBUF 2:   1 r    1      5 w r   9 w     17 w r
    S 1, KC 4, NBUF 4:   1      2      9 w     18 w    33 w         (K % 128 == 0: never ragged)
    S 4, KC 6, NBUF 5:   1 r    1 r    2 r     3       6 w r        (K / 128 = 1, 2, 9, 18, 33 tiles per split; 1 and 2 are fewer than 3 phases)
    S 4, KC 3, NBUF 4:   1 r    1 r    3       6 w     11 w

Every case prints its error / bound; the worst per mode and structure is recorded under skinny_modes/* by tests.util.observe, which
asserts it against 1.0.  No figure from an MI355X is quoted here: the module has not run on one yet."""
import pytest
import torch

from tests import skinny_ref as R
from tests.util import observe

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64
SSQ_POISON = 987654321 << 20
WINDOWS = {2: [(1, 0), (2, 0), (1, 1)],
           64: [(1, 0), (1, 5), (3, 14), (16, 0), (17, 0), (33, 0), (64, 0)],
           128: [(1, 0), (1, 5), (3, 14), (16, 0), (17, 0), (33, 0), (64, 0), (65, 0), (100, 20), (1, 127), (128, 0)]}
CAP_WINDOWS = [pytest.param(cap, win, id=f"cap{cap}-rows{win[0]}at{win[1]}") for cap, wins in WINDOWS.items() for win in wins]
_ENGINES, _PACKED = {}, {}


def engine(cap):
    if cap not in _ENGINES:
        from aurora_amd.engine import AuroraCapEngine
        _ENGINES[cap] = AuroraCapEngine({"vit": None, "llm": None}, {}, max_frames=1, max_batch=cap)
    return _ENGINES[cap]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    _PACKED.clear()


def packed(eng, cap, mode, case, K, N, w):
    """the case's weight in fragment form, gate / up rows interleaved by the loader's map; shared by every window of the capacity"""
    key = (cap, mode, case, K, N)
    if key not in _PACKED:
        if len(_PACKED) > 24:
            _PACKED.clear()
        npad = R.rup(N, 256)
        if mode == "silu_mul":
            _PACKED[key] = eng.pack(torch.cat(w), npad, K, type(eng).gateup_row_map(N // 2, npad))
        else:
            _PACKED[key] = eng.pack(w, npad, K)
    return _PACKED[key]


def struct_name(st):
    return f"wave{st.NW}" if st.kind == "wave" else f"lds_ks{st.KS}_kc{st.KC}_nbuf{st.NBUF}_s{st.S}"


def run_case(cap, mode, case, rows, b0, K, N, fold, tag="", split_min_k=8192, half=False):
    """One case through the entry: zero fill twice (determinism), then poison fill; every assertion of the module's contract.
    Returns the worst error / bound over the live outputs."""
    eng = engine(cap)
    rp = R.rup(cap, 16)
    live = slice(b0, b0 + rows)
    c = R.build_case(case, mode, rows, K, N, seed=K * 31 + N + rows * 7 + b0)
    wp = packed(eng, cap, mode, case, K, N, R.build_case(case, mode, 1, K, N, seed=K * 31 + N)["w"])
    c["w"] = R.build_case(case, mode, 1, K, N, seed=K * 31 + N)["w"]              # the weight is the shape's, the rows are the window's
    if case == "cancel":
        c["resid"] = (-(c["x"].double() @ c["w"].double().T)).half()
    g = torch.Generator().manual_seed(b0 * 131 + rows)
    ncol = N // 2 if mode == "silu_mul" else N
    if mode == "row":
        init = (torch.randn(rp, N, generator=g) * 0.5).half()
        init[live] = c["resid"]
        ssq0 = torch.randint(0, 1 << 40, (R.SSQ_SLOTS, R.MAX_BATCH), generator=g, dtype=torch.int64)
    elif mode == "silu_mul":
        init, ssq0 = torch.full((rp, ncol), -7.5, dtype=torch.float16), None
    else:
        init, ssq0 = torch.full((rp * N + GUARD,), SENTINEL, dtype=torch.float32), None
    ssq_in0 = torch.full((R.SSQ_SLOTS, R.MAX_BATCH), SSQ_POISON, dtype=torch.int64) if fold else None
    call = lambda fill: eng.decode_proj_rows(mode, c["x"], wp, N, init, b0=b0, fold=fold, eps=R.EPS, fill=fill, ssq_out=ssq0, ssq_in=ssq_in0)
    cpu = lambda r: {k: v.cpu() if v is not None else None for k, v in r.items()}
    res, again, poison = cpu(call(0.0)), cpu(call(0.0)), cpu(call(1000.0))
    where = (cap, mode, case, rows, b0, K, N, fold, tag)
    for k in res:                                                                 # determinism; live outputs independent of the dead rows
        if res[k] is not None:
            assert torch.equal(res[k], again[k]), ("not repeatable", k, where)
            assert torch.equal(res[k], poison[k]), ("depends on the dead rows' content", k, where)
    rows_view = (lambda t: t[: rp * N].view(rp, N)) if mode == "logits" else (lambda t: t)
    out, out0 = rows_view(res["out"]), rows_view(init)
    assert torch.isfinite(out.float()).all(), where
    dead = torch.ones(rp, dtype=torch.bool)
    dead[live] = False
    # ---- dead rows and everything around the live window: bitwise as the caller left it
    assert torch.equal(out[dead].view(torch.int16 if out.dtype == torch.float16 else torch.int32),
                       out0[dead].view(torch.int16 if out.dtype == torch.float16 else torch.int32)), ("a dead row was written", where)
    if mode == "logits":
        assert torch.equal(res["out"][rp * N:], init[rp * N:]), ("the guard behind the last row was written", where)
    dead_b = torch.ones(R.MAX_BATCH, dtype=torch.bool)
    dead_b[live] = False
    if mode == "row":
        assert torch.equal(res["ssq_out"][:, dead_b], ssq0[:, dead_b]), ("sum(x^2) of a dead row was touched", where)
        used = min(R.SSQ_SLOTS, N // 16)
        assert torch.equal(res["ssq_out"][used:], ssq0[used:]), ("a stripe no tile maps to was touched", where)
        if res["row_cnt"] is not None and tag.startswith("fused"):
            assert not res["row_cnt"].any(), ("arrival counters not back at zero", where)
    if fold:
        assert torch.equal(res["ssq_in"][:, dead_b], ssq_in0[:, dead_b]), ("the producer wrote sum(x^2) of a dead row", where)
        assert not res["ssq_zero"].any(), ("ssq_zero was not cleared over all stripes and rows", where)
        S, sb = R.ssq_producer_bound(c["x"])
        r = R.worst_ratio(R.ssq_value(res["ssq_in"][:, live].T), S, sb)
        observe("skinny_modes/producer_ssq_err_over_bound", r, 1.0)
    # ---- live outputs against fp64
    ref, bound = R.derived_bound(mode, c["x"], c["w"], c["resid"], fold, R.EPS)
    st = R.structure(mode, cap, K, (b0 + rows + 15) // 16, split_min_k, half)
    ratio = R.worst_ratio(out[live], ref, bound)
    print(f"{mode} {struct_name(st)} {where}: error / bound {ratio:.3f}")
    observe(f"skinny_modes/{mode}{'_fold' if fold else ''}/{struct_name(st)}_err_over_bound", ratio, 1.0)
    if mode == "row":                         # the accumulated sum(x^2) against the fp16 row the kernel returned
        S, sb = R.ssq_row_bound(out[live])
        r = R.worst_ratio(R.ssq_value((res["ssq_out"] - ssq0)[:, live].T), S, sb)
        print(f"    sum(x^2) error / bound {r:.3f}")
        observe(f"skinny_modes/row_ssq/{struct_name(st)}_err_over_bound", r, 1.0)
        ratio = max(ratio, r)
    return ratio


def rot(seq, i):
    return seq[i % len(seq)]


@pytest.mark.parametrize("cap,win", CAP_WINDOWS)
def test_residual_projection(cap, win):
    """SK_ROW: K over all five, N 64 / 320 and the three cases rotating against K and the window so that every pair meets.  The 64-slot
    engine runs per wave and, with the split threshold lowered, through split-K; split-K runs with the two-launch and the fused reduce
    (arrival counters zero afterwards); the 128-slot engine also on the half grid (two tiles per wave, from five column groups)."""
    rows, b0 = win
    wi = WINDOWS[cap].index(win)
    eng = engine(cap)
    cfgs = [("", 8192, 0, 0)]
    if cap == 64:
        cfgs += [("split", 128, 0, 0), ("fused", 128, 1, 0)]
    if cap == 128:
        cfgs += [("fused", 8192, 1, 0)] + ([("half", 8192, 0, 1)] if b0 + rows > 64 else [])
    try:
        for tag, min_k, fused, half in cfgs:
            eng.set_option("skinny_row_split_min_k", min_k)
            eng.set_option("decode_fused_reduce", fused)
            eng.set_option("decode_half_grid", half)
            for i, K in enumerate(R.K_LIST):
                run_case(cap, "row", rot(R.CASES["row"], i + wi), rows, b0, K, rot((64, 320), i + wi // 3), False, tag, min_k, bool(half))
    finally:
        eng.set_option("skinny_row_split_min_k", 8192)
        eng.set_option("decode_fused_reduce", 0)
        eng.set_option("decode_half_grid", 0)


def fold_cases(mode, i):
    """(case, fold): some cases exist only under the folded norm (skinny_ref.needs_fold)"""
    case = rot(R.CASES[mode], i)
    return case, (R.needs_fold(mode, case) or i % 2 == 0)


@pytest.mark.parametrize("cap,win", CAP_WINDOWS)
def test_gate_up_projection(cap, win):
    """SK_SILU_MUL: mlp 2176 (272 tiles: more than the CUs, so the workgroups own unequal numbers of tiles) at the two short K, 128 and
    384 elsewhere; folded norm on and off; on the 128-slot engine from five column groups also the half grid."""
    rows, b0 = win
    wi = WINDOWS[cap].index(win)
    eng = engine(cap)
    try:
        for half in ((0, 1) if cap == 128 and b0 + rows > 64 else (0,)):
            eng.set_option("decode_half_grid", half)
            for i, K in enumerate(R.K_LIST):
                mlp = 2176 if K == 128 or (K == 256 and wi % 3 == 0) else rot((128, 384), i + wi)
                case, fold = fold_cases("silu_mul", i + wi + half)
                run_case(cap, "silu_mul", case, rows, b0, K, 2 * mlp, fold, "half" if half else "", half=bool(half))
    finally:
        eng.set_option("decode_half_grid", 0)


@pytest.mark.parametrize("cap,win", CAP_WINDOWS)
def test_logits_projection(cap, win):
    """SK_LOGITS: vocabularies 320, 323 (rows end off the 16-byte grid: the column-by-column store, whose stray columns used to land in
    the next row) and 4352; every window runs 323"""
    rows, b0 = win
    wi = WINDOWS[cap].index(win)
    for i, K in enumerate(R.K_LIST):
        N = 4352 if K == 256 and wi % 2 == 0 else rot((323, 320, 323), i + wi)
        case, fold = fold_cases("logits", i + wi)
        run_case(cap, "logits", case, rows, b0, K, N, fold)


@pytest.mark.parametrize("cap", list(WINDOWS))
def test_new_entry_equals_linear_skinny(cap):
    """fold off, window at 0, zero fill: the same launch as aur_linear_skinny, bit for bit - at an odd vocabulary too"""
    eng = engine(cap)
    rp = R.rup(cap, 16)
    for rows, K, N in ((1, 128, 320), (min(cap, 17), 1152, 323), (cap, 256, 4352)):
        c = R.build_case("rand", "logits", rows, K, N, seed=K + N)
        init = torch.full((rp * N + GUARD,), SENTINEL, dtype=torch.float32)
        got = eng.decode_proj_rows("logits", c["x"], eng.pack(c["w"], R.rup(N, 256), K), N, init)["out"].cpu()
        assert torch.equal(got[: rows * N].view(rows, N), eng.linear_skinny(c["x"], c["w"]).cpu()), (rows, K, N)


@pytest.mark.parametrize("cap", [2, 64])
def test_logits_entry_takes_the_production_lm_head_route(cap):
    """The first-token logits of a 40-row prefill are, bit for bit, the "logits" mode with the folded norm applied to row 39 of the embeds
    buffer - the final hidden state the prefill left there - on an engine of 2 slots (x per wave) and of 64 (x through LDS): the entry
    and the pick path issue one launch, built in one place.  The engine keeps its packed head only as an anonymous device tensor, so the
    weight is packed again here exactly as AuroraCapEngine._load_llm does: lm_head.weight times the final norm's weight in fp32, fp16."""
    from tests.test_gpu_llm import LLM_CFGS, make_engine, padded
    cfg, L = LLM_CFGS["hd32"], 40
    d, V = cfg["hidden_size"], cfg["vocab_size"]
    eng, w = make_engine(cfg, 21, max_batch=cap)
    try:
        emb = padded(torch.randn(L, d, generator=torch.Generator().manual_seed(22)).half().float())
        eng.begin_batch(1, 4, None)
        eng.prefill(0, emb, L)
        want = eng.logits()[0].cpu()
        head = (w["lm_head.weight"].detach().to("cuda", torch.float32) * w["norm.weight"].detach().to("cuda", torch.float32)[None, :]).half()
        init = torch.full((R.rup(cap, 16) * V + GUARD,), SENTINEL, dtype=torch.float32)
        got = eng.decode_proj_rows("logits", emb[L - 1:L], eng.pack(head, R.rup(V, 256), d), V, init, fold=True, eps=cfg["rms_norm_eps"])["out"].cpu()
        assert torch.equal(got[:V].view(torch.int32), want.view(torch.int32))
    finally:
        eng.close()


def test_decode_proj_rows_rejects_bad_arguments():
    from aurora_amd._lib import AuroraHipError
    eng = engine(64)
    rp = 64
    w = eng.pack(torch.zeros(320, 128), 512, 128)
    ok = dict(x=torch.zeros(2, 128), w_packed=w, n=320, out=torch.zeros(rp, 320, dtype=torch.float16))
    bad = [dict(ok, b0=63),                                                       # the window leaves the capacity
           dict(ok, b0=-1),
           dict(ok, x=torch.zeros(65, 128)),
           dict(ok, n=330),                                                       # a residual row is whole 32-column tiles
           dict(ok, n=513),                                                       # n > npad
           dict(ok, fold=True),                                                   # no residual projection folds a norm
           dict(ok, out=torch.zeros(rp - 1, 320, dtype=torch.float16)),           # out too small for all padded rows
           dict(ok, x=torch.zeros(2, 192), w_packed=eng.pack(torch.zeros(320, 192), 512, 192))]      # k % 128
    for kw in bad:
        with pytest.raises(AuroraHipError, match="status -1"):
            eng.decode_proj_rows("row", **kw)
    with pytest.raises(AuroraHipError, match="status -1"):
        eng.decode_proj_rows("silu_mul", ok["x"], w, 352, torch.zeros(rp, 176, dtype=torch.float16))          # n % 64
    with pytest.raises(AuroraHipError, match="status -1"):
        eng.decode_proj_rows("logits", ok["x"], w, 323, torch.zeros(rp * 323, dtype=torch.float32))           # no guard behind the last row
    assert torch.isfinite(eng.decode_proj_rows("row", **ok)["out"].float()).all()                              # the ctx is still usable

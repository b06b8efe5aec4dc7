"""The prefill tile GEMMs alone - gemm_kernel (128x128) and gemm256_kernel (256x256, persistent) in every EPI_ROW epilogue mode, reached
through aur_gemm_rows - against the fp64 definition, elementwise, under the bound derived from the kernels' stated arithmetic
(tests/gemm_ref.py; nothing here is an observed tolerance).  tests/test_gemm_reference.py shows on the CPU that each of fifteen ways these
epilogues can be wrong leaves this bound by more than 10x at every launch it applies to.

Per mode variant (six activations with and without a residual, and gate-times-up) 18 (M, K, n) triples - together the 54 that hold every
pair of M in {1 .. 300}, K / 64 in {1, 2, 3, 4, 5, 7}, n in {128, 132, 256, 260, 384, 512} - each on its own case, and per triple the row

    kernel {gemm_mode 0, gemm_mode 2} x layout {wide: ldc % 8 == 0, with a partial chunk where n % 8 == 4 | ragged ldc: the 256 kernel's
    direct epilogue | row map: a permutation into a taller buffer with a quarter of the rows dropped, direct as well}

whose stored bits must all be equal, and equal to a repeated call, to gemm_nt_out 1, to every tag whose activation matches and to one
whose activation does not.  The output buffer carries extra columns, extra rows and a guard, all sentinel: any byte outside rows x
stored columns that changes fails the launch (gemm_ref.worst_ratio returns inf).  A and the residual are followed by NaN rows, A's
columns beyond K (lda > K) are NaN: a read past the operand shows as a non-finite output.

Every launch prints its error / bound; the worst per mode, kernel and epilogue is recorded under gemm_modes/* by tests.util.observe, which
asserts it against 1.0.  On an MI355X (2956 launches, 104 keys): the worst error / bound is 0.996 (gelu_tanh and relu with their fp16
output rounding at its limit; every key's worst lies between 0.984 and 0.996 - the bound's dominant term is the half-ulp of the fp16
result, which some element of a few thousand always nearly reaches), every bit-equality holds, and no kernel had to change."""
import math

import pytest
import torch

from aurora_amd import _lib
from tests import gemm_ref as R
from tests.util import observe

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
GUARD = 64                                   # halves behind the last row of the output buffer
ACT_CODE = {"none": 0, "quick_gelu": _lib.AUR_ACT_QUICK_GELU, "gelu": _lib.AUR_ACT_GELU, "silu_mul": _lib.AUR_GEMM_SILU_MUL,
            "silu": _lib.AUR_ACT_SILU, "relu": _lib.AUR_ACT_RELU, "gelu_tanh": _lib.AUR_ACT_GELU_TANH}
TAGS = _lib.GEMM_TAGS
TAGS_OF = {"none": ("vit_out", "vit_fc2", "llm_o", "llm_down"), "quick_gelu": ("vit_fc1",), "silu_mul": ("llm_gateup",)}
DEFAULTS = {"gemm_mode": 1, "gemm_max_wgs": 0, "gemm_tail_split": 1, "gemm_nt_out": -1}
_ENGINE = []


def engine():
    if not _ENGINE:
        from aurora_amd.engine import AuroraCapEngine
        _ENGINE.append(AuroraCapEngine({"vit": None, "llm": None}, {}, max_frames=1, max_batch=2))
    return _ENGINE[0]


@pytest.fixture(scope="module", autouse=True)
def _close_engine():
    yield
    for e in _ENGINE:
        e.close()
    _ENGINE.clear()


@pytest.fixture(autouse=True)
def _restore_options():
    try:
        yield
    finally:
        if _ENGINE:
            for k, v in DEFAULTS.items():
                _ENGINE[0].set_option(k, v)


class Problem:
    """One (mode, case, M, K, n): operands on the device with their NaN guards, the packed weight and bias, fp64 reference and bound"""

    def __init__(self, mode, res, case, M, K, n, lda=None):
        eng = engine()
        self.mode, self.res, self.M, self.K, self.n = mode, res, M, K, n
        c = R.build_case(case, mode, M, K, n, seed=M * 131 + K + n, with_resid=res)
        self.ref, self.bound = R.derived_bound(mode, c["a"], c["w"], c["bias"], c["resid"])
        self.npad = R.npad_of(n)
        lda = lda or K
        a = torch.full((M + 3, lda), math.nan, dtype=torch.float16)
        a[:M, :K] = c["a"]
        self.a = a.cuda()
        bias = torch.zeros(self.npad)
        if mode == "silu_mul":
            self.w = eng.pack(c["w"], self.npad, K, type(eng).gateup_row_map(n // 2, self.npad))
            bias[0:n:2], bias[1:n:2] = c["bias"][: n // 2], c["bias"][n // 2:]
        else:
            self.w = eng.pack(c["w"], self.npad, K)
            bias[:n] = c["bias"]
        self.bias = bias.cuda()
        self.resid16 = c["resid"]
        self.kernel = "k256" if self.npad % 256 == 0 else "k128"        # what gemm_mode 2 runs

    def resid(self, ldr):
        r = torch.full((self.M + 3, ldr), math.nan, dtype=torch.float16)
        r[: self.M, : self.n] = self.resid16
        return r.cuda()

    def launch(self, path, tag="other", in_place=False, ldr=None, rows=None):
        """one call; returns (buffer [R, ldc] on the CPU, guard, ref buffer, bound buffer, mask)"""
        stored, ldc = R.layout(self.mode, self.n, path)
        if path == "rows" and rows is None:
            rows = R.row_map(self.M, self.M + 37, seed=self.M + self.n)
        nrows = self.M + (37 if rows is not None else 5)
        init = torch.full((nrows * ldc + GUARD,), SENTINEL, dtype=torch.float16)
        body = init[: nrows * ldc].view(nrows, ldc)
        if in_place:
            body[: self.M, : self.n] = self.resid16
        resid = None
        if self.res and not in_place:
            resid = self.resid(ldr or R.rup(self.n, 8) + 16)
        out = engine().gemm_rows(self.a, self.w, self.n, init, m=self.M, k=self.K, ldc=ldc, bias=self.bias, act=ACT_CODE[self.mode], tag=TAGS[tag],
                                 resid=resid, in_place=in_place, out_rows=rows.int().cuda() if rows is not None else None).cpu()
        ref_buf, mask = R.scatter(self.ref, rows, body.double(), stored)
        bound_buf, _ = R.scatter(self.bound, rows, torch.zeros(body.shape, dtype=torch.float64), stored)
        return out[: nrows * ldc].view(nrows, ldc), out[nrows * ldc:], ref_buf, bound_buf, mask, rows

    def check(self, path, kernel, what="", **kw):
        """launch, assert the module's contract, return the stored values [kept rows, stored] in row order"""
        buf, guard, ref_buf, bound_buf, mask, rows = self.launch(path, **kw)
        where = (self.mode, self.res, self.M, self.K, self.n, path, kernel, what, kw.get("tag", "other"))
        assert torch.equal(guard, torch.full_like(guard, SENTINEL)), ("the guard behind the last row was written", where)
        assert torch.isfinite(buf[mask].float()).all(), ("non-finite output", where)
        ratio = R.worst_ratio(buf, ref_buf, bound_buf, mask)
        assert ratio != math.inf, ("a position outside the stored set was written", where)
        epi = {"wide": "wide_partial" if self.n % 8 == 4 else "wide", "ragged": "direct_ldc", "rows": "direct_rows"}[path]
        print(f"{where}: error / bound {ratio:.3f}")
        observe(f"gemm_modes/{self.mode}{'_res' if self.res else ''}_{kernel}_{epi}", ratio, 1.0)
        if rows is None:
            return buf[: self.M, : self.ref.shape[1]].clone()
        return buf[rows[rows >= 0], : self.ref.shape[1]].clone()


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("variant", range(len(R.VARIANTS)), ids=[f"{m}{'_res' if r else ''}" for m, r in R.VARIANTS])
def test_every_mode_on_both_kernels_and_every_epilogue_path(variant):
    mode, res = R.VARIANTS[variant]
    eng = engine()
    wrong_tag = "vit_fc1" if mode == "none" else "llm_down"                       # its activation is not this launch's: GT_OTHER must run
    for M, K, n in R.triples_of(variant):
        p = Problem(mode, res, R.case_of(M, K, n), M, K, n)
        eng.set_option("gemm_nt_out", 0)
        out = {}
        for gm, kernel in ((0, "k128"), (2, p.kernel)):
            eng.set_option("gemm_mode", gm)
            for path in R.PATHS:
                out[(gm, path)] = p.check(path, kernel)
        base = out[(0, "wide")]
        keep = None
        for (gm, path), o in out.items():
            if path == "rows":
                rows = R.row_map(M, M + 37, seed=M + n)
                keep = rows >= 0
                assert torch.equal(bits(o), bits(base[keep])), ("kernels / paths disagree", mode, res, M, K, n, gm, path)
            else:
                assert torch.equal(bits(o), bits(base)), ("kernels / paths disagree", mode, res, M, K, n, gm, path)
        # gemm_mode 2 from here on: a repeated call, the other store policy, the tagged instantiations
        assert torch.equal(bits(p.check("wide", p.kernel, "again")), bits(base)), ("not repeatable", mode, res, M, K, n)
        eng.set_option("gemm_nt_out", 1)
        assert torch.equal(bits(p.check("wide", p.kernel, "nt")), bits(base)), ("gemm_nt_out changes bits", mode, res, M, K, n)
        eng.set_option("gemm_nt_out", 0)
        for tag in TAGS_OF.get(mode, ()) + (wrong_tag,):
            for path in ("wide", "ragged"):
                assert torch.equal(bits(p.check(path, p.kernel, tag=tag)), bits(base)), ("a tag changes bits", tag, path, mode, res, M, K, n)
        eng.set_option("gemm_mode", 1)


@pytest.mark.parametrize("mode", ["none", "gelu"])
def test_residual_in_place_and_with_its_own_leading_dimension(mode):
    """resid == c (mk_pre_o, mk_pre_down) on both kernels and both layouts; beside it ldr != ldc: ldr a multiple of 8 (wide), ldr ragged
    with an aligned ldc (the direct epilogue by ldr alone), ldr == n.  All the same bits."""
    eng = engine()
    for M, K, n in ((129, 64, 256), (300, 128, 260), (257, 192, 512), (17, 256, 132)):
        p = Problem(mode, True, "rand", M, K, n)
        eng.set_option("gemm_nt_out", 0)
        outs = []
        for gm, kernel in ((0, "k128"), (2, p.kernel)):
            eng.set_option("gemm_mode", gm)
            for path in ("wide", "ragged"):
                outs.append(p.check(path, kernel, "in place", in_place=True))
                outs.append(p.check(path, kernel, "ldr wide", ldr=R.rup(n, 8) + 24))
            outs.append(p.check("wide", kernel, "ldr ragged", ldr=R.rup(n, 8) + 4))
            outs.append(p.check("wide", kernel, "ldr n", ldr=n))
            outs.append(p.check("rows", kernel, "rows"))
        keep = R.row_map(M, M + 37, seed=M + n) >= 0
        for o in outs:
            assert torch.equal(bits(o), bits(outs[0] if o.shape[0] == M else outs[0][keep])), (mode, M, K, n)


@pytest.mark.parametrize("mode", ["none", "silu_mul"])
def test_a_is_a_column_window_of_a_wider_buffer(mode):
    """lda > K: the columns of A beyond K - and the rows beyond M - are NaN"""
    eng = engine()
    for M, K, n in ((129, 64, 256), (300, 192, 512), (16, 448, 260)):
        tight, windowed = Problem(mode, False, "rand", M, K, n), Problem(mode, False, "rand", M, K, n, lda=K + 24)
        for gm, kernel in ((0, "k128"), (2, tight.kernel)):
            eng.set_option("gemm_mode", gm)
            assert torch.equal(bits(windowed.check("wide", kernel, "lda")), bits(tight.check("wide", kernel))), (mode, M, K, n, gm)


BIG_VARIANTS = (("none", False), ("none", True), ("silu_mul", False))


@pytest.mark.parametrize("kt", [1, 2, 3, 4])
def test_persistent_workgroups_walk_several_tiles_at_short_k(kt):
    """gemm_max_wgs 8, M 600, n 1024: 3 x 4 = 12 tiles on 8 workgroups, so four workgroups run a second tile whose prologue was issued
    before the first one's epilogue - at 1 and 2 K-tiles, where that prologue is the whole tile, and at 3 and 4, where the K loop's own
    staging reaches the buffers the epilogue's slabs used (W buffer 2, the second half of A buffer 1).  12 tiles are fewer than two
    rounds: launch_gemm splits nothing off.  Wide and direct epilogues, residual, gate-times-up: the bits of the 128x128 kernel."""
    eng = engine()
    for mode, res in BIG_VARIANTS:
        p = Problem(mode, res, "rand", 600, kt * 64, 1024)
        eng.set_option("gemm_nt_out", 0)
        eng.set_option("gemm_mode", 0)
        base = p.check("wide", "k128")
        eng.set_option("gemm_mode", 2)
        for wgs in (8, 0):
            eng.set_option("gemm_max_wgs", wgs)
            for path in ("wide", "ragged"):
                assert torch.equal(bits(p.check(path, "k256", f"wgs{wgs}")), bits(base)), (mode, res, kt, wgs, path)
            if res:
                assert torch.equal(bits(p.check("wide", "k256", f"wgs{wgs} in place", in_place=True)), bits(base)), (mode, kt, wgs)
        eng.set_option("gemm_max_wgs", 0)


def test_tail_split_rebases_the_row_map_and_the_residual():
    """gemm_max_wgs 8, M 4300, n 512, K 128.  launch_gemm's rule: nbn = 2, nbm = 17, tiles = 34, G = 8: full = 4 rounds, 2 tiles left;
    mfull = 4 * 8 / 2 = 16 tile rows, m0 = 4096 < M; the bottom 204 rows are small = ceil(204 / 128) * (512 / 128) = 8 tiles of the
    128x128 kernel; t_new = ceil(32 / 8) + 0.34 * ceil(8 / 8) + 0.03 = 4.37, and 4.37 + 0.1 < full + 1 = 5: rows [4096, 4300) go to
    gemm_kernel with A, the residual and C - or the row map - advanced by m0.  gemm_tail_split 0 and 1: the same bits, within the bound."""
    eng = engine()
    M, K, n = 4300, 128, 512
    eng.set_option("gemm_nt_out", 0)
    eng.set_option("gemm_mode", 2)
    eng.set_option("gemm_max_wgs", 8)
    for mode, res in BIG_VARIANTS:
        p = Problem(mode, res, "rand", M, K, n)
        outs = {}
        for split in (0, 1):
            eng.set_option("gemm_tail_split", split)
            outs[split] = [p.check("rows", "k256", f"split{split}"), p.check("wide", "k256", f"split{split}")]
            if res:
                outs[split].append(p.check("wide", "k256", f"split{split} in place", in_place=True))
                outs[split].append(p.check("ragged", "k256", f"split{split} in place", in_place=True))
        for x, y in zip(outs[0], outs[1]):
            assert torch.equal(bits(x), bits(y)), (mode, res)


def test_bad_arguments_are_refused_before_anything_is_launched():
    """every AUR_ERR_ARG rule of the entry: status -1, the output untouched, and the ctx still works"""
    eng = engine()
    L = eng.L
    M, K, n, npad = 17, 128, 256, 256
    a = torch.zeros(M, K + 8, dtype=torch.float16, device="cuda")
    w = eng.pack(torch.zeros(n, K), npad, K)
    bias = torch.zeros(npad, device="cuda")
    r = torch.zeros(M, n + 8, dtype=torch.float16, device="cuda")
    rows = torch.arange(M, dtype=torch.int32, device="cuda")
    c = torch.full((M * (n + 8) + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    ok = dict(a=a.data_ptr(), m=M, k=K, lda=K + 8, w=w.data_ptr(), npad=npad, n=n, bias=bias.data_ptr(), act=0, tag=0, resid=r.data_ptr(), ldr=n + 8,
              rows=None, c=c.data_ptr(), ldc=n + 8)
    order = ("a", "m", "k", "lda", "w", "npad", "n", "bias", "act", "tag", "resid", "ldr", "rows", "c", "ldc")

    def call(**over):
        kw = dict(ok, **over)
        rc = L.aur_gemm_rows(eng.ctx, *[kw[k] for k in order], eng._stream())
        torch.cuda.synchronize()
        return rc

    bad = [dict(k=96), dict(k=0), dict(npad=192), dict(npad=0), dict(n=130), dict(n=0), dict(n=260), dict(m=0),
           dict(lda=K - 8), dict(lda=K + 4), dict(a=a.data_ptr() + 8), dict(a=None), dict(w=None), dict(c=None),
           dict(ldc=n - 4), dict(ldc=n + 2), dict(c=c.data_ptr() + 8),
           dict(ldr=n - 4), dict(ldr=n + 2), dict(resid=r.data_ptr() + 8),
           dict(tag=1), dict(tag=5), dict(tag=9), dict(tag=-1), dict(act=7), dict(act=-1),
           dict(act=3, resid=None, ldc=n // 2 - 2), dict(act=3, resid=None, ldc=n // 2 + 1), dict(act=3),      # the last: gate-times-up with a residual
           dict(resid=c.data_ptr(), ldr=n + 4), dict(resid=c.data_ptr(), ldr=n + 8, rows=rows.data_ptr())]
    for over in bad:
        assert call(**over) == -1, over
        assert eng.L.aur_last_error(eng.ctx), over
    assert torch.equal(c, torch.full_like(c, SENTINEL)), "a refused call wrote its output"
    for over in (dict(), dict(resid=c.data_ptr(), ldr=n + 8), dict(rows=rows.data_ptr()), dict(tag=8)):
        assert call(**over) == 0, over
    body = c[: M * (n + 8)].view(M, n + 8)
    assert not body[:, :n].any() and (body[:, n:] == SENTINEL).all() and (c[M * (n + 8):] == SENTINEL).all()
    c2 = torch.full((M * (n // 2 + 2) + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    assert call(act=3, resid=None, c=c2.data_ptr(), ldc=n // 2 + 2) == 0
    body = c2[: M * (n // 2 + 2)].view(M, n // 2 + 2)
    assert not body[:, : n // 2].any() and (body[:, n // 2:] == SENTINEL).all() and (c2[M * (n // 2 + 2):] == SENTINEL).all()


def test_linear_is_the_same_launch():
    """aur_linear through the new entry's checks: the bits of aur_gemm_rows at lda = k, ldc = ldr = n, no tag - and its old answer to an
    activation it does not know (none)"""
    from aurora_amd._lib import AUR_ACT_GELU, AUR_ACT_SILU
    eng = engine()
    for M, K, n in ((129, 192, 260), (300, 64, 512)):
        c = R.build_case("rand", "gelu", M, K, n, seed=5, with_resid=True)
        got = eng.linear(c["a"], c["w"], c["bias"], act=AUR_ACT_GELU, resid=c["resid"])
        npad = R.rup(n, 256)
        bias = torch.zeros(npad)
        bias[:n] = c["bias"]
        want = eng.gemm_rows(c["a"], eng.pack(c["w"], npad, K), n, torch.zeros(M, n, dtype=torch.float16), bias=bias, act=2, resid=c["resid"])
        assert torch.equal(bits(got), bits(want)), (M, K, n)
        assert torch.equal(bits(eng.linear(c["a"], c["w"], c["bias"], act=AUR_ACT_SILU)), bits(eng.linear(c["a"], c["w"], c["bias"]))), (M, K, n)

"""Reference side of the decode-projection tests (helpers, not collected): the fp64 definitions of the three epilogue modes of the skinny
GEMM (decode.hip skinny_store: SK_ROW, SK_SILU_MUL, SK_LOGITS, with and without the folded RMSNorm), an elementwise error bound derived
from the kernels' stated arithmetic, a plain fp32 / fp16 emulator of that arithmetic with mutation switches, and the case builders.
CPU torch only; nothing here imports the product package.

Definitions, from the fp16 inputs as stored (x [rows, K], W [N, K], resid [rows, N]):
    y = x W^T;   fold: z = y * rsqrt(sum_k x_k^2 / K + eps), else z = y
    SK_LOGITS    z                                  (fp32 output)
    SK_ROW       fp16(resid + y), and sum_n out_n^2 of the fp16 row added to a 2^-28 fixed-point accumulator
    SK_SILU_MUL  fp16(silu(z_gate) * z_up)

The bound (derived_bound / ssq_row_bound / ssq_producer_bound), term by term.  u = 2^-24 (fp32), h = 2^-11 (fp16), A = sum_k |x_k| |w_k|:
  (a) accumulation: the fp16 x fp16 products are exact in fp32; each of the K additions - whatever their grouping into MFMA tiles,
      waves, k phases and split-K partials - rounds by at most u of a partial sum <= A:  e_acc = K u A   (tests.util.gemm_bound).
  (b) 1/rms.  s = sum x^2, m = s / K + eps.  The accumulator holds round(s_hat 2^28) with
        |s_hat - s| <= K u s                       the producer's fp32 sum of K exact squares (xfrag_norm_kernel, advance_tail), or
                       5 u s                       a row left by SK_ROW: 16 squares per tile = 3 in-lane additions + 2 shuffles,
        + c 2^-29                                  one round-to-nearest conversion per accumulator write: c = 1, or K / 16 tiles.
      ssq_to_rstd: (float)(double s 2^-28) [u] / (float)K [u] + eps [u], then rsqrtf [<= 2 ulp = 4 u]:
        d_m = (ds / K) / m + 3 u;   rho = |rstd_hat / rstd - 1| <= 0.55 d_m + 4 u        ((1 + d)^-1/2 - 1 <= 0.55 |d| for |d| <= 0.1)
      z_hat = y_hat rstd_hat [u]:   e_z = rstd (1 + rho) e_acc + |z| (rho + u) (1 + u)
  (c) SK_LOGITS: e_z.  SK_ROW: fp32 add then fp16:  with t = |ref| + e_acc:  e_acc + t (u + h (1 + u)) + 2^-25 (the fp16 subnormal step).
  (d) SK_SILU_MUL: silu_f(g) = g * rcp(1 + exp2(-log2(e) g)): v_exp_f32 and v_rcp_f32 are 1 ulp, the scaled argument carries 1.5 u |t|, so
        e_s = 1.1 e_g [|silu'| <= 1.1] + |silu(g)| ((1 - sigma(g)) (1.5 * 1.45 |g| u + 2 u) + 4 u);
      product [u] and fp16 [h]:  p = e_s |u| + (|silu(g)| + e_s) e_u;   bound = p + (|ref| + p) (u + h (1 + u)) + 2^-25.
  (e) SK_ROW sum(x^2), checked against the fp64 sum of the squares of the fp16 row THE KERNEL RETURNED (independent of (a)):
        (N / 16) 2^-29 + 5 u S (1 + 5 u).     A sum taken from the unrounded fp32 values falls outside it (test_skinny_reference.py).

Capacity of the accumulators.  One conversion is __float2ll_rn(p * 2^28), which saturates at 2^63: p < 2^35; the 64-bit sum of a row's
stripes wraps at 2^64 units = 2^36.  "large" rows sit at one quarter of that, 2^34; nothing is claimed beyond the limit (fp16 rows can
exceed it: 17 entries of 65504 do)."""
import math
from collections import namedtuple

import torch

from tests.util import gemm_bound, outlier_operands

U32, H16 = 2.0 ** -24, 2.0 ** -11
SSQ_SCALE = 2.0 ** 28
SSQ_SLOTS, MAX_BATCH = 16, 128
SSQ_LIMIT = 2.0 ** 36                    # sum(x^2) at which a row's 64-bit accumulator wraps
EPS = 1e-5
K_LIST = (128, 256, 1152, 2304, 4224)
MUTATIONS = ("rstd_over_n", "no_eps", "slot_dropped", "tile_ssq_dropped", "ssq_unrounded", "resid_rounded_first", "no_resid",
             "gate_up_swapped", "partial_dropped", "ragged_dropped", "dead_leak", "n4_overflow")
CASES = {"row": ("rand", "outlier", "cancel"), "silu_mul": ("rand", "outlier", "aligned", "tiny", "large"),
         "logits": ("rand", "outlier", "aligned", "tiny", "large")}


def needs_fold(mode, case):
    """tiny and large are statements about 1/rms; unnormalised outlier activations (x 1000) overflow fp16 in silu(g) * u"""
    return case in ("tiny", "large") or (mode == "silu_mul" and case == "outlier")


def rup(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------ summation structure
# kind "wave": skinny_kernel, NW waves split K interleaved (wave w: k32 = w + NW i), summed w = 0, 1, ..
# kind "lds":  skinny_lds_kernel, S k splits of K32 / S tiles each, KS k phases per tile (phase p: k32 = p mod KS inside the split, ascending),
#              phases summed p = 0, 1, .., then the splits s = 0, 1, ..; KC tiles per chunk of the x ring of NBUF buffers
Structure = namedtuple("Structure", "kind NW KS KC NBUF S")


def structure(mode, max_batch, K, nb, row_split_min_k=8192, half=False):
    """the structure launch_skinny picks (decode.hip launch_skinny_nb / launch_skx_nb) for an engine of `max_batch` slots, nb column groups.
    The library states the rule once, in mk_skinny (aurora_amd/csrc/engine.hip), for the decode step and the parity entries alike; this is
    the tests' independent statement of it."""
    variant = 1 if max_batch > 32 else 0
    if mode == "silu_mul":                      # the wide projections go through LDS at every capacity
        if max_batch > 64:                      # gu_ks == 1
            if nb > 4:
                return Structure("lds", 0, 1, 4, 4, 1) if half else Structure("lds", 0, 1, 8, 2, 1)
            return Structure("lds", 0, 1, 8, 4, 1)
        return Structure("lds", 0, 2, 8, 4, 1)
    if mode == "logits":
        return Structure("lds", 0, 1, 8 if nb <= 4 else 4, 4, 1) if variant else Structure("wave", 4, 0, 0, 0, 1)
    if variant and (K >= row_split_min_k or max_batch > 64):
        return Structure("lds", 0, 3, 6, 5, 4) if nb <= 4 else Structure("lds", 0, 3, 3, 4, 4)
    return Structure("wave", 8 if K % 256 == 0 else 4, 0, 0, 0, 1)


def chunk_table(st, K):
    """(chunks per split, does the ring wrap, is the last chunk ragged) of an "lds" structure at this K"""
    ke = K // 32 // st.S
    chunks = (ke + st.KC - 1) // st.KC
    return chunks, chunks > st.NBUF, ke % st.KC != 0


# ------------------------------------------------------------------------------------------------------------ fp64 definitions
def silu64(g):
    return g / (1.0 + torch.exp(-g))


def rstd_fp64(x, eps=EPS):
    x = x.double()
    return torch.rsqrt((x * x).sum(-1, keepdim=True) / x.shape[-1] + eps)


def reference(mode, x, w, resid=None, fold=False, eps=EPS):
    """fp64: "row" resid + y (unrounded; the fp16 rounding is in the bound); "logits" z; "silu_mul" silu(z_gate) z_up with w = (w_gate, w_up)"""
    x64 = x.double()
    r = rstd_fp64(x, eps) if fold else 1.0
    if mode == "silu_mul":
        return silu64(x64 @ w[0].double().T * r) * (x64 @ w[1].double().T * r)
    y = x64 @ w.double().T
    return resid.double() + y if mode == "row" else y * r


# ------------------------------------------------------------------------------------------------------------ the bound
def rstd_rel_err(x, eps, nconv, striped):
    """rho of (b), per row [rows, 1]"""
    x = x.double()
    K = x.shape[-1]
    s = (x * x).sum(-1, keepdim=True)
    ds = (5 if striped else K) * U32 * s + nconv * 2.0 ** -29
    d_m = ds / K / (s / K + eps) + 3 * U32
    assert float(d_m.max()) <= 0.1
    return 0.55 * d_m + 4 * U32


def _z_bound(x, w, fold, eps, striped):
    """(z fp64, e_z) of (a), (b)"""
    y = x.double() @ w.double().T
    e_acc = gemm_bound(x, w, y, False)
    if not fold:
        return y, e_acc
    r = rstd_fp64(x, eps)
    rho = rstd_rel_err(x, eps, x.shape[-1] // 16 if striped else 1, striped)
    z = y * r
    return z, r * (1 + rho) * e_acc + z.abs() * (rho + U32) * (1 + U32)


def derived_bound(mode, x, w, resid=None, fold=False, eps=EPS, striped=False):
    """(ref, bound) elementwise, shapes [rows, N] ("silu_mul": [rows, mlp]); striped: the input's sum(x^2) was left by an SK_ROW epilogue"""
    rnd = U32 + H16 * (1 + U32)
    if mode == "silu_mul":
        g, e_g = _z_bound(x, w[0], fold, eps, striped)
        u, e_u = _z_bound(x, w[1], fold, eps, striped)
        sg = silu64(g)
        sig = 1.0 / (1.0 + torch.exp(-g))
        e_s = 1.1 * e_g + sg.abs() * ((1 - sig) * (1.5 * 1.45 * g.abs() * U32 + 2 * U32) + 4 * U32)
        p = e_s * u.abs() + (sg.abs() + e_s) * e_u
        ref = sg * u
        return ref, p + (ref.abs() + p) * rnd + 2.0 ** -25
    z, e_z = _z_bound(x, w, fold, eps, striped)
    if mode == "logits":
        return z, e_z
    ref = resid.double() + z
    return ref, e_z + (ref.abs() + e_z) * rnd + 2.0 ** -25


def ssq_row_bound(out16):
    """(S, bound) of (e) for fp16 rows [rows, N] as the kernel returned them"""
    o = out16.double()
    S = (o * o).sum(-1)
    return S, (out16.shape[-1] // 16) * 2.0 ** -29 + 5 * U32 * S * (1 + 5 * U32)


def ssq_producer_bound(x):
    """(S, bound) of the producer's accumulator (one conversion)"""
    x = x.double()
    S = (x * x).sum(-1)
    return S, x.shape[-1] * U32 * S + 2.0 ** -29


def ssq_value(slots):
    """int64 [.., 16] accumulator stripes -> sum(x^2) as fp64"""
    return slots.sum(-1).double() / SSQ_SCALE


def worst_ratio(out, ref, bound):
    r = (out.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------ the emulator
def _to_fixed(p32):
    return torch.round(p32 * torch.tensor(SSQ_SCALE, dtype=torch.float32)).to(torch.int64)     # __float2ll_rn(p * SSQ_SCALE)


def emu_ssq_producer(x):
    """xfrag_norm_kernel phase 1: lane l adds the squares of its 16-byte chunks l, l + 64, .. in fp32, then the wave butterfly
    (32, 16, 8, 4, 2, 1); one conversion into stripe 0.  Returns int64 [rows, 16]."""
    rows, K = x.shape
    nch = K // 8
    sq = torch.zeros(rows, rup(nch, 64), 8, dtype=torch.float32)
    sq[:, :nch] = (x.float() * x.float()).view(rows, nch, 8)
    sq = sq.view(rows, -1, 64, 8)
    acc = torch.zeros(rows, 64, dtype=torch.float32)
    for r in range(sq.shape[1]):
        for j in range(8):
            acc = acc + sq[:, r, :, j]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    slots = torch.zeros(rows, SSQ_SLOTS, dtype=torch.int64)
    slots[:, 0] = _to_fixed(acc[:, 0])
    return slots


def emu_ssq_row(o16, vals32=None, drop_tile=None):
    """SK_ROW epilogue: per n16 tile, lane group g adds its four squares (fp32, in order), then xor16, xor32; the tile's sum goes to stripe
    tile & 15 as fixed point.  vals32: the squares are taken from these fp32 values instead of the fp16 row (mutant)."""
    rows, N = o16.shape
    v = (vals32 if vals32 is not None else o16.float()).view(rows, N // 16, 4, 4)
    sq = v * v
    p = sq[..., 0]
    for i in range(1, 4):
        p = p + sq[..., i]
    p = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
    fx = _to_fixed(p)
    slots = torch.zeros(rows, SSQ_SLOTS, dtype=torch.int64)
    for t in range(N // 16):
        if t != drop_tile:
            slots[:, t & 15] += fx[:, t]
    return slots


def emu_rstd(slots, div, eps, mut=()):
    """ssq_to_rstd: the 16 stripes as integers, (float)(double s 2^-28) / (float)K + eps, rsqrtf"""
    if "slot_dropped" in mut:
        slots = slots.clone()
        slots[:, (int((slots != 0).sum(-1).max()) - 1) & 15] = 0              # the last stripe in use
    m = (slots.sum(-1).double() / SSQ_SCALE).float() / torch.tensor(float(div), dtype=torch.float32)
    if "no_eps" not in mut:
        m = m + torch.tensor(eps, dtype=torch.float32)
    return torch.rsqrt(m)[:, None]


def sum_in_order(terms, like):
    """fp32 sum of the tensors in list order (an empty list: zeros shaped like `like`)"""
    acc = torch.zeros_like(like)
    for i, t in enumerate(terms):
        acc = t if i == 0 else acc + t
    return acc


def emu_gemm(x, w, st, mut=()):
    """y [rows, N] fp32: one fp32 partial per k32 tile (an MFMA's 32 products), accumulated in the order of `st`"""
    rows, K = x.shape
    N, K32 = w.shape[0], K // 32
    t = torch.einsum("bkc,nkc->bnk", x.float().view(rows, K32, 32), w.float().view(N, K32, 32))
    seq = lambda idx: sum_in_order([t[..., i] for i in idx], t[..., 0])
    if st.kind == "wave":
        return sum_in_order([seq(range(wv, K32, st.NW)) for wv in range(st.NW)], t[..., 0])
    ke = K32 // st.S
    full = ke // st.KC * st.KC if "ragged_dropped" in mut else ke           # mutant: the last, partly filled chunk is never consumed
    parts = [sum_in_order([seq(range(s * ke + p, s * ke + full, st.KS)) for p in range(st.KS)], t[..., 0]) for s in range(st.S)]
    return sum_in_order(parts[:-1] if "partial_dropped" in mut else parts, t[..., 0])


def silu_f(g):
    """x * rcp(1 + exp2(-log2(e) x)) in fp32"""
    return g * (1.0 / (1.0 + torch.exp2(-torch.tensor(1.4426950408889634, dtype=torch.float32) * g)))


def emulate(mode, x, w, st, resid=None, fold=False, eps=EPS, striped=False, fill=0.0, mut=()):
    """The kernels' arithmetic on the live rows x [rows, K].  Returns dict(out, ssq): out fp32 [rows, N] ("logits"), fp16 [rows, N] ("row")
    or fp16 [rows, mlp] ("silu_mul"); ssq int64 [rows, 16] = what SK_ROW adds to the accumulator stripes.  mut: names from MUTATIONS."""
    xs = x
    if "dead_leak" in mut:                      # the first live row reads a dead row's fragments
        xs = x.clone()
        xs[0] = fill
    rstd = 1.0
    if fold:
        slots = emu_ssq_row(x) if striped else emu_ssq_producer(x)
        n_all = 2 * w[0].shape[0] if mode == "silu_mul" else w.shape[0]
        rstd = emu_rstd(slots, n_all if "rstd_over_n" in mut else x.shape[1], eps, mut)
    if mode == "silu_mul":
        g, u = emu_gemm(xs, w[0], st, mut) * rstd, emu_gemm(xs, w[1], st, mut) * rstd
        if "gate_up_swapped" in mut:
            g, u = u, g
        return dict(out=(silu_f(g) * u).half(), ssq=None)
    y = emu_gemm(xs, w, st, mut) * rstd
    if mode == "logits":
        n = w.shape[0]
        if "n4_overflow" in mut and n % 4:      # the lane that owns the last columns of row b also writes the first ones of row b + 1: zeros
            y = y.clone()
            y[1:, : 4 - n % 4] = 0.0
        return dict(out=y, ssq=None)
    if "no_resid" in mut:
        v = y
    elif "resid_rounded_first" in mut:
        v = y.half().float() + resid.float()
    else:
        v = y + resid.float()
    o = v.half()
    ssq = emu_ssq_row(o, v if "ssq_unrounded" in mut else None, 1 if "tile_ssq_dropped" in mut else None)
    return dict(out=o, ssq=ssq)


def applies(mutation, mode, st, K, N, rows, fold, striped):
    """does `mutation` change the arithmetic of this shape at all"""
    if mutation in ("rstd_over_n", "no_eps"):
        return fold and (mutation == "no_eps" or N != K)
    if mutation == "slot_dropped":
        return fold and striped
    if mutation in ("tile_ssq_dropped", "ssq_unrounded", "no_resid"):
        return mode == "row"
    if mutation == "resid_rounded_first":
        # what it changes is at most 2^-12 |y|, and the bound is at least K 2^-24 |y|: visible at 10x only while K < 2^12 / 10
        return mode == "row" and K * 10 < 4096
    if mutation == "gate_up_swapped":
        return mode == "silu_mul"
    if mutation == "partial_dropped":
        return st.kind == "lds" and st.S > 1
    if mutation == "ragged_dropped":
        return st.kind == "lds" and chunk_table(st, K)[2]
    if mutation == "n4_overflow":
        return mode == "logits" and N % 4 != 0 and rows > 1
    return mutation == "dead_leak"


# ------------------------------------------------------------------------------------------------------------ cases
def build_case(name, mode, rows, K, N, seed):
    """dict(x [rows, K], w [N, K] or (w_gate, w_up) [N / 2, K] each, resid [rows, N] or None), fp16.
    rand: N(0, 0.5^2) activations, N(0, 0.05^2) weights.  outlier: one activation column x 1000, 0.1 % of the weights x 20.
    aligned: non-negative operands, no cancellation inside the dot product (A = |y|: the accumulation term is K 2^-24 |y|, its smallest;
    added because a 3 % error of 1/rms - one accumulator stripe of sixteen lost - stayed within 6.5x of the bound of "rand" at K = 4224).
    cancel ("row"): aligned operands and resid = -fp16(y): the output is the fp16 rounding residue of y.  tiny (fold): every second row's entries are fp16 subnormals around 2^-20: the squares vanish below the 2^-28
    quantum and 1/rms -> rsqrt(eps).  large (fold): every second row has sum(x^2) = 2^34, a quarter of the accumulators' capacity."""
    g = torch.Generator().manual_seed(seed)
    if name == "outlier":
        x, w = outlier_operands(rows, N, K, g)
    else:
        x = (torch.randn(rows, K, generator=g) * 0.5).half()
        w = (torch.randn(N, K, generator=g) * 0.05).half()
    if name in ("cancel", "aligned"):
        x, w = x.abs(), w.abs()
    elif name == "tiny":
        x[::2] = (torch.randn((rows + 1) // 2, K, generator=g) * 2.0 ** -20).half()
        w = (w.float() * 20).half()
    elif name == "large":
        a = math.sqrt(SSQ_LIMIT / 4 / K)
        x[::2] = (torch.sign(torch.randn((rows + 1) // 2, K, generator=g)) * a).half()
    resid = None
    if mode == "row":
        resid = (torch.randn(rows, N, generator=g) * 0.5).half()
        if name == "cancel":
            resid = (-(x.double() @ w.double().T)).half()
    if mode == "silu_mul":
        w = (w[: N // 2].contiguous(), w[N // 2:].contiguous())
    return dict(x=x, w=w, resid=resid)

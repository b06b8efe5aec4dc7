"""Reference side of the prefill tile-GEMM tests (helpers, not collected): the fp64 definitions of the EPI_ROW epilogue modes of
gemm_kernel / gemm256_kernel (gemm_epilogue.h gemm_epilogue<EPI_ROW>, gemm256.hip g2_epilogue_row_u), an elementwise error bound derived
from the kernels' stated arithmetic, a plain fp32 / fp16 emulator of that arithmetic with mutation switches, and the case builders.
CPU torch only; nothing here imports the product package.

Definitions, from the fp16 inputs as stored (a [M, K], w [n, K], bias fp32 [n], resid [M, n]):
    z = a w^T + bias
    none z | quick_gelu z sigma(1.702 z) | gelu 0.5 z (1 + erf(z / sqrt 2)) | gelu_tanh 0.5 z (1 + tanh(sqrt(2 / pi) (z + 0.044715 z^3)))
    silu z sigma(z) | relu max(z, 0)                   each: fp16(f(z) + resid), the residual added AFTER the activation (resid optional)
    silu_mul   fp16(silu(z_gate) * z_up), w = [gate rows; up rows] (n / 2 each; the packed weight interleaves them), n / 2 columns stored
    out_rows   row i of the result lands in row out_rows[i] of the output buffer; a negative entry drops the row

The bound (derived_bound), term by term.  u = 2^-24 (fp32), h = 2^-11 (fp16), A = sum_k |a_k| |w_k|:
  (a) accumulation: the fp16 x fp16 products are exact in fp32; each of the K additions - whatever their grouping into MFMAs and K-tiles -
      rounds by at most u of a partial sum <= A:  e_acc = K u A   (tests.util.gemm_bound).
  (b) bias: one fp32 add:  e_z = e_acc + u (|z| + e_acc).
  (c) activation f evaluated at the computed z_hat:  e_f = L e_z + eval(x), x = |z| + e_z, L the Lipschitz constant of f:
        none, relu      L = 1, eval = 0
        silu (c = 1), quick_gelu (c = 1.702): x * rcp(1 + exp2(-c log2(e) x)) - tests/skinny_ref.py item (d) with the factor c on the scaled
                        argument:  L = 1.1 (max |f'| = 1.0998 for both: f(x) = silu(c x) / c),
                        eval = |f| ((1 - sigma(c z)) (1.5 * 1.45 c x u + 2 u) + 4 u)
        gelu            L = 1.13 (max of Phi(x) + x phi(x) = 1.129 at x = sqrt 2).  The error of 1 + erf(..) is ABSOLUTE - the sum cancels
                        for negative x - so it is carried as 0.5 x c u:  erff within 16 ulp <= 32 u (|erf| <= 1), the argument x / sqrt 2
                        (constant + product: 1.5 u relative) moves erf by at most |t erf'(t)| 1.5 u <= 0.75 u, the add rounds by <= 2 u:
                        c = 35;  the last product rounds by u |f|:   eval = 0.5 x 35 u + u |f|
        gelu_tanh       L = 1.13.  tanhf within 5 ulp <= 10 u; the argument sqrt(2 / pi) (x + 0.044715 x^3) carries <= 6 u relative (two
                        products, a constant, a product, an add of equal signs, a constant product) and |t tanh'(t)| <= 0.45: 3 u; the add 2 u:
                        c = 15:   eval = 0.5 x 15 u + u |f|
      The ulp limits are the OpenCL full-profile ones OCML implements (erf 16 ulp, tanh 5 ulp): the ROCm documentation installed beside
      the compiler states none for erff / tanhf.
  (d) residual: one fp32 add:  e_v = e_f + u (|ref| + e_f),  ref = f(z) + resid.
  (e) output: one rounding to fp16:  bound = e_v + (|ref| + e_v) h + 2^-25 (half the fp16 subnormal step).
  (f) silu_mul: e_s of silu(g) as in (c); product [u] and fp16 [h] as skinny_ref (d):
        p = e_s |up| + (|silu(g)| + e_s) e_up;   bound = p + (|ref| + p) (u + h (1 + u)) + 2^-25.
Positions of the output buffer the launch must not store - columns [stored, ldc), rows outside the map, dropped rows, the guard - have
bound 0 against the buffer's initial content: worst_ratio returns inf when one of them changed.

K-tiles.  Both kernels step K by 64.  gemm_kernel double-buffers its stage (K-tile kt in buffer kt % 2: first reuse at K / 64 = 3);
gemm256_kernel double-buffers A (first reuse at 3) and triple-buffers W (first reuse at 4), and its prologue takes a different path at
K / 64 = 1 (nothing of K-tile 1 staged) and 2 (no K-tile 2): KT_LIST = 1, 2, 3, 4, 5, 7 holds every one of these counts."""
import math

import torch

from tests.util import gemm_bound, outlier_operands

U32, H16 = 2.0 ** -24, 2.0 ** -11
ACTS = ("none", "quick_gelu", "gelu", "gelu_tanh", "silu", "relu")
MODES = ACTS + ("silu_mul",)
CASES = ("rand", "outlier", "cancel", "spread")
M_LIST = (1, 16, 17, 127, 128, 129, 255, 257, 300)
KT_LIST = (1, 2, 3, 4, 5, 7)
N_LIST = (128, 132, 256, 260, 384, 512)
MUTATIONS = ("bias_dropped", "bias_shift16", "resid_before_act", "resid_wrong_block", "resid_ignored", "gate_up_swapped", "mul_at_n",
             "out_rows_ignored", "dropped_row_to_0", "map_not_rebased", "last_ktile_dropped", "ktile_twice", "erf_tanh_swapped",
             "quick_silu_swapped", "partial_upper_stored")
SQRT_2_OVER_PI = 0.7978845608028654


def rup(x, m):
    return (x + m - 1) // m * m


def npad_of(n):
    """the packed width the tests use: 128 for one tile, else whole 256-column tiles - except 384, which only the 128x128 kernel takes"""
    return n if n in (128, 384) else rup(n, 256)


def triples():
    """54 (M, K, n) holding every (M, K), (M, n) and (K, n) pair of the three lists: n index = (i + j) mod 6"""
    return [(M, kt * 64, N_LIST[(i + j) % 6]) for i, M in enumerate(M_LIST) for j, kt in enumerate(KT_LIST)]


def triples_of(variant):
    """the 18 triples mode variant `variant` (an integer) runs: (i - j) mod 3 == variant mod 3 - every M, every K and every n among them"""
    t = triples()
    return [t[i * 6 + j] for i in range(9) for j in range(6) if (i - j) % 3 == variant % 3]


def case_of(M, K, n):
    """the case a triple runs: (i + 2 j) mod 4 - every variant's 18 triples hold each case at least four times"""
    return CASES[(M_LIST.index(M) + 2 * KT_LIST.index(K // 64)) % 4]


VARIANTS = tuple((m, r) for m in ACTS for r in (False, True)) + (("silu_mul", False),)       # (mode, with a residual)
PATHS = ("wide", "ragged", "rows")


def layout(mode, n, path):
    """(stored columns, ldc) of an epilogue path.  wide: ldc % 8 == 0 (% 4 for silu_mul) with at least 8 (4) columns beyond the stored
    ones - n % 8 == 4 makes the last chunk partial; ragged: ldc % 8 == 4 (% 4 == 2), which sends the 256x256 kernel to its direct
    epilogue - the stored width itself where that is ragged (n = 132, 260), else 12 (6) columns more than the rounded width;
    rows: the wide buffer, written through a row map (direct as well)"""
    mul = mode == "silu_mul"
    stored, q = (n // 2, 4) if mul else (n, 8)
    if path == "ragged":
        return stored, stored if stored % q == q // 2 else rup(stored, q) + q + q // 2
    return stored, rup(stored, q) + q


# ------------------------------------------------------------------------------------------------------------ fp64 definitions
def act64(mode, z):
    if mode == "none":
        return z
    if mode == "relu":
        return z.clamp(min=0.0)
    if mode in ("silu", "quick_gelu"):
        return z / (1.0 + torch.exp(-(1.702 if mode == "quick_gelu" else 1.0) * z))
    if mode == "gelu":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    assert mode == "gelu_tanh", mode
    return 0.5 * z * (1.0 + torch.tanh(SQRT_2_OVER_PI * (z + 0.044715 * z ** 3)))


def preact64(a, w, bias):
    z = a.double() @ w.double().T
    return z + bias.double() if bias is not None else z


def reference(mode, a, w, bias=None, resid=None):
    """fp64 [M, stored columns], unrounded (the fp16 rounding is in the bound)"""
    z = preact64(a, w, bias)
    if mode == "silu_mul":
        h = z.shape[1] // 2
        return act64("silu", z[:, :h]) * z[:, h:]
    y = act64(mode, z)
    return y + resid.double() if resid is not None else y


def scatter(rows, out_rows, init, stored):
    """rows [M, stored] into a copy of init [R, ldc] (any dtype) through the row map; returns (buffer, mask of the stored positions)"""
    buf = init.clone()
    mask = torch.zeros(init.shape, dtype=torch.bool)
    idx = torch.arange(rows.shape[0]) if out_rows is None else torch.as_tensor(out_rows, dtype=torch.long)
    keep = idx >= 0
    buf[idx[keep], :stored] = rows[keep].to(init.dtype)
    mask[idx[keep], :stored] = True
    return buf, mask


# ------------------------------------------------------------------------------------------------------------ the bound
def _act_err(mode, z, e_z):
    """(f(z), e_f) of (c)"""
    f = act64(mode, z)
    x = z.abs() + e_z
    if mode in ("none", "relu"):
        return f, e_z
    if mode in ("silu", "quick_gelu"):
        c = 1.702 if mode == "quick_gelu" else 1.0
        sig = 1.0 / (1.0 + torch.exp(-c * z))
        return f, 1.1 * e_z + f.abs() * ((1 - sig) * (1.5 * 1.45 * c * x * U32 + 2 * U32) + 4 * U32)
    return f, 1.13 * e_z + 0.5 * x * (35 if mode == "gelu" else 15) * U32 + U32 * f.abs()


def derived_bound(mode, a, w, bias=None, resid=None):
    """(ref, bound) elementwise fp64 [M, stored columns]"""
    z = preact64(a, w, bias)
    e_acc = gemm_bound(a, w, z, False)
    e_z = e_acc + (U32 * (z.abs() + e_acc) if bias is not None else 0.0)
    if mode == "silu_mul":
        h = z.shape[1] // 2
        sg, e_s = _act_err("silu", z[:, :h], e_z[:, :h])
        up, e_u = z[:, h:], e_z[:, h:]
        p = e_s * up.abs() + (sg.abs() + e_s) * e_u
        ref = sg * up
        return ref, p + (ref.abs() + p) * (U32 + H16 * (1 + U32)) + 2.0 ** -25
    f, e_f = _act_err(mode, z, e_z)
    ref, e_v = f, e_f
    if resid is not None:
        ref = f + resid.double()
        e_v = e_f + U32 * (ref.abs() + e_f)
    return ref, e_v + (ref.abs() + e_v) * H16 + 2.0 ** -25


def worst_ratio(buf, ref_buf, bound_buf, mask):
    """max over the stored positions of |buf - ref| / bound; inf when a stored value is not finite or a position outside `mask` differs
    from ref_buf (there ref_buf holds the initial content, bit for bit)"""
    if not torch.equal(buf[~mask].view(torch.int16), ref_buf[~mask].to(buf.dtype).view(torch.int16)):
        return math.inf
    r = (buf[mask].double() - ref_buf[mask]).abs() / bound_buf[mask]
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------ the emulator
def emu_acc(a, w, kmut=None):
    """fp32 [M, n]: one fp32 partial per 32 columns of K (an MFMA's products), accumulated in ascending k.  kmut "last_ktile_dropped": the
    last 64 columns never arrive; "ktile_twice": the last K-tile is read from the previous one's buffer (a stale stage)"""
    M, K = a.shape
    a32, w32 = a.float().clone(), w.float().clone()
    if kmut == "last_ktile_dropped":
        a32[:, K - 64:] = 0.0
    elif kmut == "ktile_twice":
        a32[:, K - 64:], w32[:, K - 64:] = a32[:, K - 128:K - 64].clone(), w32[:, K - 128:K - 64].clone()
    t = torch.einsum("mkc,nkc->mnk", a32.view(M, K // 32, 32), w32.view(w.shape[0], K // 32, 32))
    acc = t[..., 0]
    for i in range(1, K // 32):
        acc = acc + t[..., i]
    return acc


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def act32(mode, v):
    """the device functions of common.h in fp32"""
    if mode == "none":
        return v
    if mode == "relu":
        return v.clamp(min=0.0)
    if mode in ("silu", "quick_gelu"):
        k = _f32(2.4554669595930157 if mode == "quick_gelu" else 1.4426950408889634)
        return v * (1.0 / (1.0 + torch.exp2(-k * v)))
    if mode == "gelu":
        return _f32(0.5) * v * (1.0 + torch.erf(v * _f32(0.70710678118654752)))
    return _f32(0.5) * v * (1.0 + torch.tanh(_f32(SQRT_2_OVER_PI) * (v + _f32(0.044715) * v * v * v)))


def emulate(mode, a, w, bias, resid, out_rows, init, n, mut=(), m0=0, acc=None):
    """The kernels' arithmetic into a copy of the output buffer init [R, ldc] fp16.  n: the width (interleaved for silu_mul; w holds
    [gate; up]).  m0: rows from m0 on go to a second launch whose row map is re-based by m0 (the tail split).  acc: emu_acc(a, w) when the
    caller has it.  mut: names from MUTATIONS."""
    M = a.shape[0]
    kmut = next((m for m in ("last_ktile_dropped", "ktile_twice") if m in mut), None)
    v = emu_acc(a, w, kmut) if acc is None or kmut else acc
    if bias is not None and "bias_dropped" not in mut:
        b = bias.float()
        if "bias_shift16" in mut:
            b = torch.roll(b, -16)
        v = v + b
    if mode == "silu_mul":
        g, up = v[:, : n // 2], v[:, n // 2:]
        if "gate_up_swapped" in mut:
            g, up = up, g
        o, stored = (act32("silu", g) * up).half(), n // 2
    else:
        fn = mode
        if "erf_tanh_swapped" in mut:
            fn = {"gelu": "gelu_tanh", "gelu_tanh": "gelu"}.get(mode, mode)
        if "quick_silu_swapped" in mut:
            fn = {"silu": "quick_gelu", "quick_gelu": "silu"}.get(mode, mode)
        r = None
        if resid is not None and "resid_ignored" not in mut:
            r = resid.float()
            if "resid_wrong_block" in mut:             # the next 16-row block's rows, clamped to the last row
                r = r[torch.clamp(torch.arange(M) + 16, max=M - 1)]
        if r is not None and "resid_before_act" in mut:
            o = act32(fn, v + r).half()
        else:
            o = (act32(fn, v) + r if r is not None else act32(fn, v)).half()
        stored = n
    idx = torch.arange(M) if out_rows is None or "out_rows_ignored" in mut else torch.as_tensor(out_rows, dtype=torch.long).clone()
    if "map_not_rebased" in mut and out_rows is not None and 0 < m0 < M:
        idx[m0:] = idx[: M - m0].clone()
    if "dropped_row_to_0" in mut:
        idx = idx.clamp(min=0)
    buf = init.clone()
    keep = idx >= 0
    if "mul_at_n" in mut and mode == "silu_mul":       # column j stored at the interleaved index 2 j
        cols = torch.arange(0, min(2 * stored, init.shape[1]), 2)
        buf[idx[keep][:, None], cols] = o[keep][:, : cols.numel()]
        return buf
    if "dropped_row_to_0" in mut:
        for i in torch.arange(M)[keep].tolist():       # in row order: a later row wins, as a later store would
            buf[idx[i], :stored] = o[i]
    else:
        buf[idx[keep], :stored] = o[keep]
    if "partial_upper_stored" in mut:                  # the chunk's upper half: zero weight rows and zero bias -> act(0) (+ nothing) = 0
        buf[idx[keep], stored:stored + (2 if mode == "silu_mul" else 4)] = 0.0
    return buf


def applies(mutation, mode, M, K, n, ldc, bias, resid, out_rows, m0=0, case="rand"):
    """does `mutation` change the stored bits of this launch at all - and, for the two activation exchanges, visibly at 10x"""
    mul = mode == "silu_mul"
    if mutation in ("bias_dropped", "bias_shift16"):
        return bias
    if mutation == "resid_ignored":
        return resid and not mul
    if mutation == "resid_before_act":
        # relu on "cancel": resid = -relu(z) is 0 where z < 0 and cancels z where z > 0 - both orders leave the rounding residue
        return resid and mode not in ("none", "silu_mul") and not (mode == "relu" and case == "cancel")
    if mutation == "resid_wrong_block":
        return resid and not mul and M > 1
    if mutation in ("gate_up_swapped", "mul_at_n"):
        return mul
    if mutation in ("out_rows_ignored", "dropped_row_to_0"):
        return out_rows
    if mutation == "map_not_rebased":
        return out_rows and 0 < m0 < M
    if mutation == "last_ktile_dropped":
        return True
    if mutation == "ktile_twice":
        return K >= 128
    if mutation == "erf_tanh_swapped":
        # the two GELUs differ by <= 5e-4, relatively most in the negative tail: under the fp16 rounding of the bulk ("rand", "cancel":
        # |z| < 2) and the accumulation term of "outlier" they stay inside 10x; "spread" puts z over [-6, 6] with a small A
        return mode in ("gelu", "gelu_tanh") and case == "spread"
    if mutation == "quick_silu_swapped":
        return mode in ("silu", "quick_gelu")
    if mutation == "partial_upper_stored":
        return n % 8 == 4 and ldc >= (n // 2 + 2 if mul else n + 4)
    raise KeyError(mutation)


# ------------------------------------------------------------------------------------------------------------ cases
def build_case(name, mode, M, K, n, seed, with_resid=False):
    """dict(a [M, K], w [n, K] ("silu_mul": gate rows then up rows), bias fp32 [n], resid [M, n] or None), fp16 operands.
    Every case scales the rows of a by a ramp 0.5 .. 1.5 and the rows of w by 1.5 .. 0.5: the result is far from symmetric, a transposed
    or row / column-exchanged store cannot pass.
    rand: N(0, 0.5^2) activations, N(0, 0.05^2) weights, N(0, 0.3^2) bias.  outlier: tests.util.outlier_operands (one activation column
    x 1000, 0.1 % of the weights x 20); for silu_mul the activations x 0.1, so that silu(gate) * up stays below 65504.
    cancel: rand with resid = -fp16(f(z)): the output is the rounding residue (silu_mul has no residual: rand).
    spread: the accumulation is small (std 0.02) and the bias ramps over [-6, 6] across the columns, in a shuffled order: pre-activations
    cover the tails of the activations where A, and so the bound, is small (silu_mul: the gate bias ramps, the up bias is 1 +- 0.3)."""
    g = torch.Generator().manual_seed(seed)
    if name == "outlier":
        a, w = outlier_operands(M, n, K, g)
        a, w = a.float() * (0.1 if mode == "silu_mul" else 1.0), w.float()
    else:
        a = torch.randn(M, K, generator=g) * 0.5
        w = torch.randn(n, K, generator=g) * (0.04 / math.sqrt(K) if name == "spread" else 0.05)
    a = (a * torch.linspace(0.5, 1.5, M)[:, None]).half()
    w = (w * torch.linspace(1.5, 0.5, n)[:, None]).half()
    bias = torch.randn(n, generator=g) * 0.3
    if name == "spread":
        m = n // 2 if mode == "silu_mul" else n
        ramp = torch.linspace(-6.0, 6.0, m)[torch.randperm(m, generator=g)]
        bias = torch.cat([ramp, 1.0 + bias[m:]]) if mode == "silu_mul" else ramp
    resid = None
    if with_resid and mode != "silu_mul":
        resid = (torch.randn(M, n, generator=g) * 0.5).half()
        if name == "cancel":
            resid = (-reference(mode, a, w, bias)).half()
    return dict(a=a, w=w, bias=bias.float(), resid=resid)


def row_map(M, R, seed):
    """int64 [M]: a permutation of M rows into rows 1 .. R - 1 of a taller buffer, about a quarter dropped (-1) - among them the first and
    the last row of every 16-row block.  Row 0 of the buffer is nobody's target: a dropped row stored there (the clamp of a negative
    index) shows as a lost sentinel"""
    g = torch.Generator().manual_seed(seed)
    rm = 1 + torch.randperm(R - 1, generator=g)[:M]
    drop = torch.rand(M, generator=g) < 0.2
    drop[0::16] = True
    drop[15::16] = True
    drop[M - 1] = True
    rm[drop] = -1
    return rm

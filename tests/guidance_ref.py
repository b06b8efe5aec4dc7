"""Classifier-free guidance: an fp32 restatement of `guidance_apply_kernel`'s stated arithmetic, the bound of its result against the
float64 definition (`aurora_amd.guidance.apply`), shared cases, and deliberately wrong variants.  No GPU, no torch.

The kernel's arithmetic (aurora_amd/csrc/guidance.hip), u = 2^-24 the unit roundoff of fp32, V the vocabulary, for each of the two rows
(x = c or u, R_x = max x - min x its spread):

    m      = max x                                   exact
    d_i    = fl(x_i - m)                             |err| <= u |d_i| <= u R_x
    e_i    = expf(d_i)                               relative error <= EXP_ULPS ulp = 2 EXP_ULPS u of exp(d_i), and exp(d_i (1 + delta))
                                                     moves e_i by a relative |d_i| u
    S^     = sum e_i in score_row_stats' tree        a thread adds its ceil(V / 4096) quads of 4 in turn, then 6 + 4 butterfly levels:
                                                     DEPTH = 4 ceil(V / 4096) + 10 additions deep; all terms are positive, so the
                                                     relative error of the sum is <= DEPTH u
    L^     = logf(S^)                                <= LOG_ULPS ulp of log S^

Relative error of S^ against S = sum exp(x_i - m): the per-term errors weigh in with p_i = e_i / S, so
    |S^ / S - 1| <= (DEPTH + 2 EXP_ULPS + sum_i p_i |d_i|) u,   and   sum_i p_i |d_i| = H(p) - log S <= log V
because log p_i = d_i - log S, H(p) <= log V and S >= 1 (the maximum contributes exp(0)).  Terms below the fp32 exponent range
(d_i < -87) may flush to zero: at most V 2^-126 absolutely, nothing beside S >= 1.  log is 1-Lipschitz in relative terms, log S <= log V:
    E_log(V) = |L^ - log S| <= (DEPTH + 2 EXP_ULPS + log V) u + 2 LOG_ULPS u log V
    lx_i   = fl(d_i - L^)                            |lx_i| <= R_x + log V
    E_l(x) = |lx_i - exact| <= u R_x + E_log(V) + u (R_x + log V)
Then, with T = R_c + R_u + 2 log V >= |lc_i - lu_i|, the three explicitly rounded operations:
    t      = fl(lc_i - lu_i)                         rounding <= u T, carried into the result times |g|
    p      = fl(g t)                                 rounding <= u |g| T
    out_i  = fl(p + lu_i)                            rounding <= u |out_i| <= u (|g| T + R_u + log V)
and since out = g lc + (1 - g) lu, the errors of lc and lu arrive scaled by |g| and |g - 1|:

    bound(c, u, g) = [ |g| E_l(c) + |g - 1| E_l(u) + u (3 |g| T + R_u + log V) ] (1 + SECOND_ORDER)

EXP_ULPS = LOG_ULPS = 2 (the device library documents 1 ulp for expf and logf; numpy's float32 exp / log, which the restatement
below uses, stay within the same), SECOND_ORDER = 1e-3 covers the products of two errors.  Nothing here was fitted to an observation.
"""
import numpy as np

from aurora_amd import guidance as GD
from aurora_amd import logit_rules as LR

U = 2.0 ** -24
EXP_ULPS = 2
LOG_ULPS = 2
SECOND_ORDER = 1e-3
THREADS = 1024
SCALES = (0.5, 1.5, 3.0, 7.5)


def depth(V: int) -> int:
    return 4 * -(-V // (4 * THREADS)) + 10


def e_log(V: int) -> float:
    lv = np.log(V)
    return (depth(V) + 2 * EXP_ULPS + lv) * U + 2 * LOG_ULPS * U * lv


def e_l(row) -> float:
    r = np.asarray(row, np.float64)
    R, lv = float(r.max() - r.min()), np.log(r.shape[0])
    return U * R + e_log(r.shape[0]) + U * (R + lv)


def bound(c, u, g: float) -> float:
    """max-abs bound of the kernel's guided row against `guidance.apply(c, u, g)` in float64 (the derivation is this file's docstring)"""
    c, u = np.asarray(c, np.float64), np.asarray(u, np.float64)
    lv = np.log(c.shape[0])
    Ru = float(u.max() - u.min())
    T = float(c.max() - c.min()) + Ru + 2 * lv
    g = abs(float(g))
    return (g * e_l(c) + abs(float(np.float32(g)) - 1.0) * e_l(u) + U * (3 * g * T + Ru + lv)) * (1 + SECOND_ORDER)


def tree_sum(e: np.ndarray) -> np.float32:
    """sum of an fp32 row in score_row_stats' order: element 4 q + j belongs to thread q % 1024, which adds its elements in increasing
    order; 64 lanes join in a butterfly (32 .. 1), the 16 wave sums in a second one (8 .. 1)"""
    V = e.shape[0]
    nq = -(-V // 4)
    rounds = -(-nq // THREADS)
    pad = np.zeros(rounds * THREADS * 4, np.float32)
    pad[:V] = e
    pad = pad.reshape(rounds, THREADS, 4)
    s = np.zeros(THREADS, np.float32)
    for r in range(rounds):
        for j in range(4):
            s = (s + pad[r, :, j]).astype(np.float32)          # adding the padding's 0.0 changes nothing
    s = s.reshape(THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lane ^ o]).astype(np.float32)
    w = s[:, 0].copy()
    wl = np.arange(THREADS // 64)
    for o in (8, 4, 2, 1):
        w = (w + w[wl ^ o]).astype(np.float32)
    return np.float32(w[0])


def log_softmax32(row) -> np.ndarray:
    x = np.asarray(row, np.float32)
    d = (x - x.max()).astype(np.float32)
    with np.errstate(under="ignore"):
        L = np.float32(np.log(tree_sum(np.exp(d).astype(np.float32))))
    return (d - L).astype(np.float32)


def kernel_apply(c, u, g: float) -> np.ndarray:
    """The kernel's arithmetic in numpy float32: every operation rounded on its own, no contraction"""
    lc, lu = log_softmax32(c), log_softmax32(u)
    t = (lc - lu).astype(np.float32)
    p = (np.float32(g) * t).astype(np.float32)
    return (p + lu).astype(np.float32)


def apply_rows(buf, recs, b0: int = 0, nb=None, fn=GD.apply):
    """What the apply launch over rows [b0, b0 + nb) leaves: (buffer, save) - a leader's row guided, its original in its save row
    (NaN elsewhere); every other row as it was.  float64.  Every leader reads the INPUT rows (pairs are disjoint)."""
    buf = np.asarray(buf, np.float32)
    out = buf.astype(np.float64)
    save = np.full(buf.shape, np.nan)
    nb = len(buf) - b0 if nb is None else nb
    for b in range(b0, b0 + nb):
        g = float(recs["scale"][b])
        if g > 0 and g != 1 and np.isfinite(g):
            out[b] = fn(buf[b], buf[int(recs["partner"][b])], g)
            save[b] = buf[b]
    return out, save


def row_pair(rng, V: int, sigma: float = 4.0, boosts: int = 6, boost: float = 12.0, shared: float = 0.7):
    """A conditional and an unconditional row as a model gives them: N(0, sigma^2) with some boosted tokens; the unconditional row
    shares part of the conditional one (the language prior) and has boosted tokens of its own"""
    c = rng.normal(0.0, sigma, V)
    u = shared * c + np.sqrt(1 - shared * shared) * rng.normal(0.0, sigma, V)
    c[rng.integers(0, V, boosts)] += boost * rng.random(boosts)
    u[rng.integers(0, V, boosts)] += boost * rng.random(boosts)
    return c.astype(np.float32), u.astype(np.float32)


def cases(n_per: int = 3, vocabs=(32000, 1003), seed: int = 20):
    """[(tag, c, u, g)]: seeded pairs over both vocabularies and every scale, plus a pair of identical rows and a pair whose spread of
    200 lets the exp underflow"""
    out = []
    for V in vocabs:
        for gi, g in enumerate(SCALES):
            for k in range(n_per):
                rng = np.random.default_rng(seed + 1000 * V + 10 * gi + k)
                c, u = row_pair(rng, V)
                out.append((f"v{V}_g{g}_{k}", c, u, g))
            rng = np.random.default_rng(seed + 7 * V + gi)
            c, _ = row_pair(rng, V)
            out.append((f"v{V}_g{g}_identical", c, c.copy(), g))
            w, _ = row_pair(rng, V)
            w = (w * np.float32(200.0 / (w.max() - w.min()))).astype(np.float32)
            out.append((f"v{V}_g{g}_spread200", w, c, g))
    return out


# ---- single mistakes: each is `guidance.apply` (float64) with one thing wrong
def _lse(x):
    x = np.asarray(x, np.float64)
    return x.max() + np.log(np.exp(x - x.max()).sum())


def wrong_raw_u(c, u, g):
    lc = GD.log_softmax(c)
    return g * (lc - np.asarray(u, np.float64)) + np.asarray(u, np.float64)


def wrong_swapped(c, u, g):
    return GD.apply(u, c, g)


def wrong_minus(c, u, g):
    return g * GD.log_softmax(c) - GD.log_softmax(u)


def wrong_max(c, u, g):
    c, u = np.asarray(c, np.float64), np.asarray(u, np.float64)
    lc = (c - u.max()) - np.log(np.exp(c - c.max()).sum())          # the partner's maximum under the leader's sum
    return g * (lc - GD.log_softmax(u)) + GD.log_softmax(u)


def wrong_no_shift(c, u, g):
    c = np.asarray(c, np.float64)
    lc = (c - c.max()) - np.log(np.exp(c).sum())                    # S without the shift, the row with it
    return g * (lc - GD.log_softmax(u)) + GD.log_softmax(u)


def wrong_weights(c, u, g):
    lc, lu = GD.log_softmax(c), GD.log_softmax(u)
    return (g - 1) * (lc - lu) + lu                                 # g and g - 1 confused: the weights (g - 1, 2 - g)


def wrong_partner_sum(c, u, g):
    c, u = np.asarray(c, np.float64), np.asarray(u, np.float64)
    lc = GD.log_softmax(c)
    lu = (u - u.max()) - np.log(np.exp(c - c.max()).sum())          # the partner's row under the leader's sum
    return g * (lc - lu) + lu


def wrong_no_normalise(c, u, g):
    c, u = np.asarray(c, np.float64), np.asarray(u, np.float64)
    return g * (c - u) + u                                          # raw rows throughout


ROW_MISTAKES = dict(raw_u=wrong_raw_u, rows_swapped=wrong_swapped, g_lc_minus_lu=wrong_minus, wrong_rows_maximum=wrong_max,
                    sum_without_shift=wrong_no_shift, weights_g_minus_1=wrong_weights, partner_under_leaders_sum=wrong_partner_sum,
                    no_log_softmax=wrong_no_normalise)


def chain(c, u, g, history, rules, eos_id, guidance_first: bool = True):
    """guidance, then the logit rules (transformers' order) - or, with guidance_first=False, the mistake: rules, then guidance"""
    if guidance_first:
        return LR.apply(GD.apply(c, u, g).astype(np.float32), history, rules, eos_id).astype(np.float64)
    return GD.apply(LR.apply(c, history, rules, eos_id), u, g)

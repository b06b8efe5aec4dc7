"""CPU: the reference side of tests/test_gpu_gemm_modes.py checks itself.  The emulator of the EPI_ROW epilogues' arithmetic
(tests/gemm_ref.py emulate) must stay inside the derived bound on every launch of the GPU module - every mode variant, its 18 (M, K, n)
triples with the case each one runs, the three epilogue layouts, the persistent multi-tile shape and the tail-split shape - and every
mutant of it must leave the bound by more than 10x on at least one element of EVERY launch it applies to (gemm_ref.applies), so that the
GPU test, which asserts error <= 1.0 x bound and untouched sentinels, cannot pass a kernel with one of these defects.

erf_tanh_swapped applies to the "spread" case only: the two GELUs differ by at most 5e-4, and where |z| < 2 ("rand", "cancel") the fp16
rounding of the output, or with "outlier" the accumulation term, covers that within 10x; "spread" holds pre-activations over [-6, 6] at a
small sum |a| |w|, and every GELU variant meets it at four or more of its triples.  resid_before_act leaves out relu on "cancel", where
both orders give the rounding residue.  The row map never targets row 0 of the output buffer, so dropped_row_to_0 always costs a sentinel.

Results (this module prints them; `pytest -s`), 732 launches:
  emulator, worst error / bound per mode: 0.988 (silu_mul) .. 0.996 (gelu_tanh, relu).
  smallest margin of each mutant over the launches it applies to (x bound):
    bias_dropped 2.0e3       bias_shift16 5.2e3        resid_before_act 1.7e3     resid_wrong_block 1.1e4    resid_ignored 5.4e3
    gate_up_swapped 1.1e3    mul_at_n 1.7e6            out_rows_ignored inf       dropped_row_to_0 inf       map_not_rebased 7.8e5
    last_ktile_dropped 490   ktile_twice 662           erf_tanh_swapped 24        quick_silu_swapped 629     partial_upper_stored inf
  (inf: a sentinel outside the stored set was overwritten)."""
import functools
import math

import pytest
import torch

from tests import gemm_ref as R

MARGIN = 10.0
SENTINEL = -7.5
# (M, K, n, m0): the persistent multi-tile shape at its four K, and the tail-split shape with the row the split starts at
BIG = tuple((600, kt * 64, 1024, 0) for kt in (1, 2, 3, 4)) + ((4300, 128, 512, 4096),)
BIG_VARIANTS = (("none", False), ("none", True), ("silu_mul", False))


def launches():
    """(mode, with_resid, M, K, n, case, path, m0) of every launch shape of the GPU module"""
    out = []
    for v, (mode, res) in enumerate(R.VARIANTS):
        for M, K, n in R.triples_of(v):
            out += [(mode, res, M, K, n, R.case_of(M, K, n), path, 0) for path in R.PATHS]
    for mode, res in BIG_VARIANTS:
        for M, K, n, m0 in BIG:
            out += [(mode, res, M, K, n, "rand", path, m0) for path in (("wide", "rows") if m0 else ("wide", "ragged"))]
    return out


@functools.lru_cache(maxsize=64)
def _case(case, mode, M, K, n, res):
    c = R.build_case(case, mode, M, K, n, seed=M * 131 + K + n, with_resid=res)
    c["acc"] = R.emu_acc(c["a"], c["w"])
    c["ref"], c["bound"] = R.derived_bound(mode, c["a"], c["w"], c["bias"], c["resid"])
    return c


def evaluate(launch, mut=()):
    mode, res, M, K, n, case, path, m0 = launch
    c = _case(case, mode, M, K, n, res)
    stored, ldc = R.layout(mode, n, path)
    rows = R.row_map(M, M + 37, seed=M + n) if path == "rows" else None
    init = torch.full((M + (37 if path == "rows" else 5), ldc), SENTINEL, dtype=torch.float16)
    ref_buf, mask = R.scatter(c["ref"], rows, init.double(), stored)
    bound_buf, _ = R.scatter(c["bound"], rows, torch.zeros(init.shape, dtype=torch.float64), stored)
    buf = R.emulate(mode, c["a"], c["w"], c["bias"], c["resid"], rows, init, n, mut, m0, c["acc"])
    return R.worst_ratio(buf, ref_buf, bound_buf, mask)


@functools.lru_cache(maxsize=None)
def survey():
    """(worst unmutated ratio per mode, {mutation: (smallest ratio over the launches it applies to, that launch, their number)})"""
    worst = {}
    margins = {m: (math.inf, None, 0) for m in R.MUTATIONS}
    for launch in launches():
        mode, res, M, K, n, case, path, m0 = launch
        worst[mode] = max(worst.get(mode, 0.0), evaluate(launch))
        _, ldc = R.layout(mode, n, path)
        for m in R.MUTATIONS:
            if R.applies(m, mode, M, K, n, ldc, True, res, path == "rows", m0, case):
                if path == "rows" and M == 1:
                    continue                              # the one row is dropped: nothing is stored, nothing can differ
                r = evaluate(launch, (m,))
                lo, at, cnt = margins[m]
                margins[m] = (r, launch, cnt + 1) if r < lo else (lo, at, cnt + 1)
    return worst, margins


def test_the_emulator_stays_inside_the_bound():
    worst, _ = survey()
    print("emulator worst error / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == set(R.MODES)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutant_leaves_the_bound_on_every_launch_it_applies_to(mutation):
    _, margins = survey()
    lo, at, n = margins[mutation]
    print(f"{mutation}: smallest margin {lo:.3g} x bound at {at}, {n} launches")
    assert n > 0, "the mutation applies to no launch of the survey"
    assert lo > MARGIN, (mutation, lo, at)


def test_the_triples_hold_every_pair_and_every_variant_every_value():
    t = R.triples()
    assert len(t) == 54 and len(set(t)) == 54
    for x, y, nx, ny in ((0, 1, 9, 6), (0, 2, 9, 6), (1, 2, 6, 6)):
        assert len({(s[x], s[y]) for s in t}) == nx * ny
    for v in range(len(R.VARIANTS)):
        tv = R.triples_of(v)
        assert len(tv) == 18
        assert {s[0] for s in tv} == set(R.M_LIST) and {s[1] // 64 for s in tv} == set(R.KT_LIST) and {s[2] for s in tv} == set(R.N_LIST)
        assert sum(R.case_of(*s) == "spread" for s in tv) >= 4 and {R.case_of(*s) for s in tv} == set(R.CASES)


def test_the_k_list_holds_every_staging_ring_edge():
    """gemm_kernel: 2 stages; gemm256_kernel: 2 A buffers, 3 W buffers, prologue branches at 1 and 2 K-tiles"""
    for depth in (2, 3):
        assert depth + 1 in R.KT_LIST                     # the first K-tile that lands in a buffer used before
    assert {1, 2} <= set(R.KT_LIST) and max(R.KT_LIST) >= 2 * 3 + 1       # the longer ring wraps twice


def test_layouts_select_the_paths_they_are_named_after():
    for mode in ("none", "silu_mul"):
        q = 4 if mode == "silu_mul" else 8
        for n in R.N_LIST + (1024,):
            stored, wide = R.layout(mode, n, "wide")
            _, ragged = R.layout(mode, n, "ragged")
            assert wide % q == 0 and wide >= stored + q and ragged % q == q // 2 and ragged >= stored
            assert ragged == stored or stored % q == 0
    assert R.layout("none", 132, "ragged") == (132, 132) and R.layout("silu_mul", 260, "ragged") == (130, 130)


def test_the_row_map_drops_block_edges_and_about_a_quarter():
    for M in (16, 129, 300, 4300):
        rm = R.row_map(M, M + 37, seed=M)
        kept = rm[rm >= 0]
        assert len(set(kept.tolist())) == kept.numel() and 1 <= int(kept.min()) and int(kept.max()) < M + 37
        assert (rm[0::16] < 0).all() and (rm[15::16] < 0).all() and rm[M - 1] < 0
        if M >= 129:
            assert 0.2 <= float((rm < 0).float().mean()) <= 0.4

"""CPU: the sampling definition (aurora_amd/sampling.py) against its known answers and against transformers' own warpers, its draw
statistics, and the argument handling of every way in (engine, model, CLI, lmms plugin).  No GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from aurora_amd import sampling as S
from tests.sampling_cases import SETTINGS, chi2_stat, golden_cases, make_row
from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- 1. the generator
def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{x:08x}" for x in S.philox4x32_10(ctr, key)) == want


def test_uniform_is_a_24_bit_fraction_and_depends_on_every_argument():
    us = [S.uniform(1234567890123, 5, n) for n in range(512)]
    assert all(0.0 <= u < 1.0 and (u * 2 ** 24) == int(u * 2 ** 24) for u in us)
    assert len(set(us)) > 500
    base = S.uniform(7, 3, 11)
    assert base != S.uniform(7, 3, 12) and base != S.uniform(7, 4, 11) and base != S.uniform(8, 3, 11)
    assert base != S.uniform(7 + (1 << 32), 3, 11)                 # the seed's high word is the second key word
    assert S.uniform(7, 3, 11) == (S.philox4x32_10((11, 3, 0, 0), (7, 0))[0] >> 8) * 2.0 ** -24


# ------------------------------------------------------------------------------------------- 2. the kept set vs transformers' warpers
def _hf_mask(row, T, k, p, dtype=torch.float64):
    from tests.golden.make_golden_sampling import hf_kept
    return torch.isfinite(hf_kept(torch.from_numpy(row).to(dtype), T, k, p)).numpy()


def test_kept_set_sizes_equal_the_stored_hf_float64_sizes_on_all_2560_rows():
    g = golden("g18_sampling.npz")
    cases = golden_cases()
    assert len(cases) == 2560 and g["seeds"].tolist() == [c[1] for c in cases]
    assert int(g["sets_differ"]) == 0 and (g["kept_f64"] == g["kept_f32"]).all()      # HF float32 and float64 keep the same sets
    assert 0 < float(g["f32_cdf_dev"]) < 1e-5
    for i, seed, sigma, (T, k, p) in cases:
        assert int(S.kept_mask(make_row(seed, sigma), T, k, p).sum()) == int(g["kept_f64"][i]), (i, seed, sigma, T, k, p)


def test_kept_set_equals_transformers_float64_warpers():
    """the sets themselves, live, on every 8th row (every setting and sigma)"""
    for i, seed, sigma, (T, k, p) in golden_cases()[::8]:
        row = make_row(seed, sigma)
        assert (S.kept_mask(row, T, k, p) == _hf_mask(row, T, k, p)).all(), (i, seed, T, k, p)


def test_repeated_values_at_the_boundary_stand_or_fall_together():
    # top-k: the k-th largest value repeats -> both copies stay (transformers keeps ties at the threshold too)
    row = np.full(16, -5.0, np.float32)
    row[[2, 9, 11]] = [3.0, 2.0, 2.0]
    keep = S.kept_mask(row, 1.0, 2, 1.0)
    assert np.nonzero(keep)[0].tolist() == [2, 9, 11] and (keep == _hf_mask(row, 1.0, 2, 1.0)).all()
    # top-p: probabilities 0.4, 0.2, 0.2, 0.2 and p = 0.5.  The values strictly above the three equal ones weigh 0.4 < 0.5: all three
    # stay.  transformers sorts and cuts between equal values (keeps the maximum and ONE of them): the documented difference
    row = np.log(np.array([0.2, 0.4, 0.2, 0.2], np.float64)).astype(np.float32)
    keep = S.kept_mask(row, 1.0, 0, 0.5)
    assert keep.tolist() == [True, True, True, True]
    assert int(_hf_mask(row, 1.0, 0, 0.5).sum()) == 2
    # ... and they fall together when what lies above them already holds p: 0.6, 0.2, 0.2 with p = 0.5 keeps the maximum alone
    row = np.log(np.array([0.2, 0.6, 0.2], np.float64)).astype(np.float32)
    assert S.kept_mask(row, 1.0, 0, 0.5).tolist() == [False, True, False]
    tok, kept, _ = S.reference_pick(row, 1.0, 0, 0.5, 1, 2, 3)
    assert (tok, kept) == (1, 1)
    # temperature 0: greedy, the FIRST maximum
    assert S.reference_pick(np.array([1.0, 7.0, 7.0, 0.0], np.float32), 0, 50, 0.9, 0, 0, 0)[:2] == (1, 1)


# --------------------------------------------------------------------------------------------------------- 3. the draw's statistics
@pytest.mark.parametrize("setting", [(0.7, 50, 0.9), (1.0, 0, 0.9), (1.5, 0, 0.5)])
def test_reference_frequencies_follow_its_own_probabilities(setting):
    from scipy.stats import chi2
    T, k, p = setting
    row = make_row(424242, 4.0)
    keep = S.kept_mask(row, T, k, p)
    idx, lo, hi = S.cdf_intervals(row, T, keep)
    N = 65536
    u = np.array([S.uniform(1234567890123, 5, n) for n in range(N)])
    pos = np.searchsorted(hi, u, side="right")                  # first kept token whose cumulative mass exceeds u
    for n in (0, 1, 777, N - 1):                                # ... which is what reference_pick returns
        assert S.reference_pick(row, T, k, p, 1234567890123, 5, n)[0] == idx[min(pos[n], len(idx) - 1)]
    counts = np.bincount(np.minimum(pos, len(idx) - 1), minlength=len(idx))
    stat, dof = chi2_stat(counts, hi - lo, N)
    assert dof >= 1 and stat < chi2.ppf(1 - 1e-6, dof), (stat, dof)


def test_the_gpu_suites_flat_model_separates_seeds_and_streams_within_eight_tokens():
    """tests/test_gpu_sampling.py asserts that different seeds / streams give different ids on the tiny hd32 model (weights seed 5,
    T = 1, top-p 0.95).  Chosen here, on the CPU: the reference rolled out on the oracle's own logits of that model differs within
    the first 8 tokens for every prompt the GPU test uses first."""
    from oracle import aurora_oracle as O
    from tests.test_gpu_llm import LLM_CFGS
    from tests.util import rand_llm_weights
    cfg = LLM_CFGS["hd32"]
    w = rand_llm_weights(cfg, 5)

    def rollout(emb, seed, stream):
        x, out = emb, []
        for n in range(8):
            h, _ = O.llama_forward(x, w, cfg, None, 0)
            logits = torch.nn.functional.linear(h[-1:], w["lm_head.weight"])[0].float().numpy()
            out.append(S.reference_pick(logits, 1.0, 0, 0.95, seed, stream, n)[0])
            x = torch.cat([x, w["embed_tokens.weight"][out[-1]][None]], 0)
        return out
    for i in range(3):
        emb = torch.randn(40 + 7 * i, cfg["hidden_size"], generator=torch.Generator().manual_seed(i)).half().float()
        a = rollout(emb, 11, i)
        assert a != rollout(emb, 12, i) and a != rollout(emb, 11, 100 + i), i
        assert len(set(a)) >= 4                                   # flat enough: the draws spread


# ------------------------------------------------------------------------------------------------------------ 4. argument handling
def test_check_sampling_validates_like_transformers():
    assert S.check_sampling(None) is None
    assert S.check_sampling(dict(temperature=0.7)) == dict(temperature=0.7, top_k=50, top_p=1.0, seed=0)
    assert S.check_sampling(dict(temperature=1, top_k=None, top_p=None, seed=9)) == dict(temperature=1.0, top_k=0, top_p=1.0, seed=9)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=1.0, top_p=0.0),
                dict(temperature=1.0, top_p=1.5), dict(temperature=1.0, top_k=-1), dict(temperature=1.0, seed=-1),
                dict(temperature=1.0, topp=0.9)):
        with pytest.raises(ValueError):
            S.check_sampling(bad)


def test_records_layout_is_the_headers_struct():
    from aurora_amd import _lib
    src = open(os.path.join(ROOT, "include", "aurora_hip.h")).read()
    body = re.search(r"typedef struct aur_sampling \{(.*?)\} aur_sampling;", src, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            ctype, names = decl.split(" ", 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ct = {"float": C.c_float, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    assert [(n, t) for n, t in _lib.AurSampling._fields_] == [(n, ct[t]) for n, t in fields]
    assert C.sizeof(_lib.AurSampling) == 24 == S.RECORD.itemsize
    assert list(S.RECORD.names) == [n for n, _ in fields]
    assert [S.RECORD.fields[n][1] for n in S.RECORD.names] == [getattr(_lib.AurSampling, n).offset for n, _ in fields]
    r = S.records(dict(temperature=0.5, top_k=7, top_p=0.25, seed=(1 << 40) + 3), [4, 9])
    as_c = _lib.AurSampling.from_buffer_copy(r[1:2].tobytes())
    assert (as_c.temperature, as_c.top_p, as_c.top_k, as_c.stream, as_c.seed) == (0.5, 0.25, 7, 9, (1 << 40) + 3)
    assert not S.records(None, [0, 1, 2]).view(np.uint8).any()                 # greedy records are all zero bits (temperature 0)
    for name in ("aur_slot_sampling", "aur_sample_rows"):
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", src)


class _FakeEngine:
    dev, max_new_tokens, l = "cpu", 64, {"hidden_size": 8}

    def __init__(self):
        self.calls = []

    def generate(self, embeds, lens, n, eos_id=2, **kw):
        self.calls.append(kw)
        return [[1, 2, 3]]


def test_llm_generate_argument_handling():
    from aurora_amd.model import _LLM
    e = _FakeEngine()
    llm = _LLM(e, 2)
    x = torch.zeros(1, 5, 8)
    llm.generate(inputs_embeds=x, do_sample=False, temperature=0.7, top_p=0.9)          # transformers ignores them without do_sample
    assert e.calls[-1] == {}
    llm.generate(inputs_embeds=x, do_sample=True, temperature=0.7, top_p=0.9)
    assert e.calls[-1] == dict(sampling=dict(temperature=0.7, top_k=50, top_p=0.9, seed=0), streams=[0])
    llm.generate(inputs_embeds=x, do_sample=True, temperature=1.0, top_k=0, seed=5, stream=3)
    assert e.calls[-1] == dict(sampling=dict(temperature=1.0, top_k=0, top_p=1.0, seed=5), streams=[3])
    llm.generation_top_k = 20                                                         # the checkpoint's generation_config.json wins over 50
    llm.generate(inputs_embeds=x, do_sample=True, temperature=1.0)
    assert e.calls[-1]["sampling"]["top_k"] == 20
    llm.generate(inputs_embeds=x, do_sample=True, temperature=1.0, top_k=3)
    assert e.calls[-1]["sampling"]["top_k"] == 3
    n = len(e.calls)
    for bad in (dict(temperature=0.0), dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=1.1), dict(temperature=1.0, top_k=-2)):
        with pytest.raises(ValueError):
            llm.generate(inputs_embeds=x, do_sample=True, **bad)
    with pytest.raises(NotImplementedError):
        llm.generate(inputs_embeds=x, do_sample=True, temperature=1.0, num_beams=4)
    assert len(e.calls) == n


def test_generation_top_k_is_read_from_the_checkpoint(tmp_path):
    from aurora_amd.model import generation_top_k
    assert generation_top_k(str(tmp_path)) is None
    (tmp_path / "llm").mkdir()
    (tmp_path / "llm" / "generation_config.json").write_text('{"top_k": 40, "temperature": 0.9}')
    assert generation_top_k(str(tmp_path)) == 40
    assert generation_top_k(os.path.join(ROOT, "tests", "golden", "ckpt_tiny")) is None


def test_cli_flags():
    import inference
    a = inference.build_parser().parse_args([])
    assert (a.do_sample, a.top_k, a.seed, a.temperature, a.top_p) == (False, 50, 0, 0.0, 1.0)
    a = inference.build_parser().parse_args(["--do_sample", "--temperature", "0.7", "--top_p", "0.9", "--top_k", "0", "--seed", "11"])
    assert (a.do_sample, a.top_k, a.seed, a.temperature, a.top_p) == (True, 0, 11, 0.7, 0.9)
    import subprocess
    import sys
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--do_sample"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--temperature" in bad.stderr and "Traceback" not in bad.stderr
    text = inference.build_parser().format_help()
    assert "greedy only" not in text and "unused" not in text


# ---- the lmms plugin, with the fakes of tests/test_lmms_plugin.py plus a model that records what it was asked
def _plugin(sampling_model, **kw):
    from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
    from tests.test_lmms_plugin import FakeTok, fake_pre
    return P, P.AuroraCapMI355X(pretrained="unused", device="cpu", batch_size=2, _model=sampling_model, _tokenizer=FakeTok(),
                                _preprocessor=fake_pre, **kw)


class _BatchModel:
    def __init__(self):
        self.visual_encoder = SimpleNamespace(reset_tome_r=lambda r: None)
        self.calls = []

    def caption_batch(self, clips, max_new_tokens=2048, **kw):
        self.calls.append((len(clips), kw))
        return [[7] for _ in clips]


class _StreamModel(_BatchModel):
    def caption_stream(self, clips, max_new_tokens=2048, on_error=None, **kw):
        got = []
        for k, _ in enumerate(clips):
            got.append(kw["stream_of"](k) if "stream_of" in kw else None)
            yield k, [7]
        self.calls.append((got, {a: b for a, b in kw.items() if a != "stream_of"}))


def _requests(gens):
    docs = {i: np.zeros((2, 8, 8, 3), np.uint8) for i in range(len(gens))}
    return docs, [SimpleNamespace(args=("x" * (1 + (i * 3) % 5), g, lambda d: [d], i, "t", "s")) for i, g in enumerate(gens)]


def test_plugin_sampling_is_opt_in_and_streams_are_request_indices():
    P, m = _plugin(_BatchModel())
    assert m.sampling is False and m.seed == 0
    with pytest.raises(NotImplementedError):
        P.gen_defaults({"temperature": 0.7})
    with pytest.raises(NotImplementedError):
        P.gen_defaults({"temperature": 0.7, "num_beams": 2}, sampling=True)
    g = P.gen_defaults({"temperature": 0.7}, sampling=True)
    assert g["do_sample"] is True and g["top_p"] == 1.0 and g["temperature"] == 0.7              # top_p None -> 1.0
    assert "do_sample" not in P.gen_defaults({"temperature": 0}, sampling=True)
    gens = [{"temperature": 0.7, "top_p": 0.9}, {}, {"temperature": 0.7, "top_p": 0.9}, {"temperature": 0.7, "top_p": 0.9}, {}]
    docs, reqs = _requests(gens)
    m.task_dict = {"t": {"s": docs}}
    with pytest.raises(NotImplementedError):
        m.generate_until(reqs)                                                                   # built without sampling=True
    for model in (_BatchModel(), _StreamModel()):
        P, m = _plugin(model, sampling="True", seed=7)                                           # --model_args hands strings over
        assert m.sampling is True and m.seed == 7
        m.task_dict = {"t": {"s": docs}}
        assert m.generate_until(reqs) == ["7"] * 5
        want = dict(temperature=0.7, top_p=0.9, seed=7)
        if isinstance(model, _StreamModel):
            sampled = [c for c in model.calls if c[1]]
            greedy = [c for c in model.calls if not c[1]]
            assert len(sampled) == 1 and sampled[0][1] == dict(sampling=want) and sorted(sampled[0][0]) == [0, 2, 3]
            assert len(greedy) == 1 and greedy[0][0] == [None, None]
        else:
            sampled = [kw for _, kw in model.calls if kw]
            assert all(kw["sampling"] == want for kw in sampled)
            assert sorted(s for kw in sampled for s in kw["streams"]) == [0, 2, 3]               # whatever the batching
            assert sum(n for n, kw in model.calls if not kw) == 2                                # temperature 0 stays greedy
    with pytest.raises(NotImplementedError):
        m.loglikelihood([])

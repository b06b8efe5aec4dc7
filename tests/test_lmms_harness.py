"""CPU: the adaptor driven by what the REFERENCE's own lmms-eval harness hands it, replayed from fixture G16.

tests/golden/make_golden_harness.py runs the reference harness over an in-memory task with this adaptor behind it (plugin import,
`register_model`, `create_from_arg_string`, `ConfigurableTask.build_all_requests`, `evaluator.evaluate`) and records the keyword
arguments the constructor received, the arguments of every `generate_until` request in the harness's order, and the response the
harness's `process_results` saw per document.  Here the same requests go through the adaptor again, with the fake engine of
tests/test_lmms_plugin.py: its "caption" encodes (frames, prompt ids, markers), so every document must get ITS OWN response, in the
harness's order, whatever order the adaptor batched in - and exactly the response the harness delivered when the fixture was made."""
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np

from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
from tests.test_lmms_plugin import FakeModel, FakeTok, fake_pre

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _docs():
    spec = importlib.util.spec_from_file_location("make_golden_harness", os.path.join(GOLDEN, "make_golden_harness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.docs()


def test_reference_harness_drives_the_adaptor():
    g = np.load(os.path.join(GOLDEN, "g16_lmms_harness.npz"))
    init_kwargs = json.loads(str(g["init_kwargs"]))
    calls = json.loads(str(g["generate_until_calls"]))
    delivered = {i: r for i, r in json.loads(str(g["responses_by_doc"]))}
    frames, questions = _docs()
    n_docs = len(questions)

    fake = FakeModel()
    lm = P.AuroraCapMI355X(**init_kwargs, _model=fake, _tokenizer=FakeTok(), _preprocessor=fake_pre)
    assert lm.token_merge_ratio == 0.3 and lm.max_frames_num == 4 and lm.batch_size == 3
    assert lm.rank == 0 and lm.world_size == 1
    lm.task_dict = {"tiny_vdc": {"test": [{"idx": i, "question": questions[i]} for i in range(n_docs)]}}

    def expected(i):                                                                  # what the fake engine answers for document i
        prompt = P.conv_prompt(P.question_with_image_tokens(questions[i], len(frames[i])))
        ids = P.tokenizer_image_token(prompt, FakeTok())
        return " ".join(map(str, [len(frames[i]), len(ids), len(frames[i])]))

    got = {}
    for call in calls:
        reqs = [SimpleNamespace(args=(ctx, gen, lambda doc: [frames[doc["idx"]]], doc_id, task, split)) for ctx, gen, doc_id, task, split in call]
        out = lm.generate_until(reqs)
        assert len(out) == len(reqs)
        for (_, _, doc_id, _, _), resp in zip(call, out):                             # the harness: req.resps.append(resp), in request order
            assert doc_id not in got
            got[doc_id] = resp
    assert sorted(got) == list(range(n_docs)) == sorted(delivered)
    for i in range(n_docs):
        assert got[i] == expected(i) == delivered[i], (i, got[i], expected(i), delivered[i])
    assert sum(n for n, _ in fake.calls) == n_docs                                    # every request reached the engine exactly once
    assert all(m == 8 for _, m in fake.calls)                                         # the harness's generation_kwargs
    assert fake.visual_encoder.ratio == 0.3

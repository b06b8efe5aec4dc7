#!/usr/bin/env python3
"""G16 - what the reference's own lmms-eval harness hands the adaptor, recorded so that tests/test_lmms_harness.py replays it without
the harness.  The harness is imported from the reference tree; its third-party imports that the image lacks (loguru, evaluate,
sqlitedict, tenacity, sacrebleu, hf_transfer) are stubbed, nothing of lmms_eval itself is.  Then, as `lmms_eval` does:
  * `LMMS_EVAL_PLUGINS=aurora_amd.lmms_plugin` -> `lmms_eval/models/__init__.py:62-70` imports our module, whose class registers
    itself through the reference's `register_model` (api/registry.py:11-24, which asserts it extends `lmms`);
  * `get_model(name).create_from_arg_string(model_args, {"batch_size": .., "device": ..})` (evaluator.py simple_evaluate);
  * a real `ConfigurableTask` (api/task.py:605) over an in-memory dataset builds the `Instance` requests
    (`task.build_all_requests`), and `evaluator.evaluate` runs them: `getattr(lm, "generate_until")(cloned_reqs)`,
    `req.resps.append`, filters, `process_results`, aggregation (evaluator.py:406-457, 519-546).
The engine behind the adaptor is a fake (tests/test_lmms_plugin.py): its "caption" encodes (frames, prompt ids, markers), so every
document's response names the request it came from.  Recorded: the keyword arguments `create_from_arg_string` gave the constructor,
the arguments of every `generate_until` request in the harness's order, and the response `process_results` received per document.

    python tests/golden/make_golden_harness.py <reference lmms-eval directory>      (CPU, seconds)
"""
import importlib
import json
import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
N_DOCS = 7
MODEL_ARGS = "pretrained=unused,token_merge_ratio=0.3,max_frames_num=4"
ADDITIONAL = {"batch_size": 3, "device": "cpu"}


def docs():
    """the in-memory task: frames and questions per document (the test rebuilds the same from this function's rule)"""
    rng = np.random.default_rng(0)
    frames = {i: rng.integers(0, 255, (1 + i % 3, 8, 8, 3), dtype=np.uint8) for i in range(N_DOCS)}
    questions = ["describe clip %d " % i + "x" * (3 * (i % 4)) for i in range(N_DOCS)]
    return frames, questions


def import_harness(ref):
    sys.path.insert(0, ref)

    def stub(name, **attrs):
        if name in sys.modules:
            return
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m

    lg = logging.getLogger("lmms-eval")

    class _Logger:
        def __getattr__(self, n):
            return getattr(lg, "info" if n == "success" else n, lg.info)

        def remove(self, *a, **k):
            pass

        def add(self, *a, **k):
            return 0

    class _Stop:
        def __or__(self, other):
            return self

    stub("loguru", logger=_Logger())
    stub("evaluate", load=lambda *a, **k: None)
    stub("sqlitedict", SqliteDict=dict)
    stub("tenacity", retry=lambda *a, **k: (lambda f: f), stop_after_attempt=lambda *a, **k: _Stop(), stop_after_delay=lambda *a, **k: _Stop(),
         wait_fixed=lambda *a, **k: None)
    stub("sacrebleu")
    stub("hf_transfer")
    os.environ["LMMS_EVAL_PLUGINS"] = "aurora_amd.lmms_plugin"
    importlib.import_module("lmms_eval.models")                                      # runs the plugin loop (models/__init__.py:62-70)
    return importlib.import_module("lmms_eval.api.registry"), importlib.import_module("lmms_eval.api.task"), \
        importlib.import_module("lmms_eval.evaluator")


def main():
    ref = os.path.abspath(sys.argv[1])
    sys.path.insert(0, ROOT)
    import datasets
    registry, task_mod, evaluator = import_harness(ref)
    from lmms_eval.api.model import lmms
    from tests.test_lmms_plugin import FakeModel, FakeTok, fake_pre
    P = importlib.import_module("aurora_amd.lmms_plugin.models.auroracap_mi355x")
    cls = registry.get_model("auroracap_mi355x")                                     # the reference's registry lookup
    assert cls is P.AuroraCapMI355X and issubclass(cls, lmms)

    init_kwargs, calls = {}, []
    init, gen_until = cls.__init__, cls.generate_until

    def rec_init(self, **kw):
        init_kwargs.update({k: v for k, v in kw.items() if not k.startswith("_")})
        init(self, **kw)

    def rec_generate_until(self, requests):
        calls.append([[a[0], a[1], a[3], a[4], a[5]] for a in (r.args for r in requests)])
        return gen_until(self, requests)

    cls.__init__, cls.generate_until = rec_init, rec_generate_until
    lm = cls.create_from_arg_string(MODEL_ARGS, dict(ADDITIONAL, _model=FakeModel(), _tokenizer=FakeTok(), _preprocessor=fake_pre))
    frames, questions = docs()

    class InMemoryCaptionTask(task_mod.ConfigurableTask):
        def download(self, dataset_kwargs=None):                                      # the one thing the reference would fetch from the hub
            ds = datasets.Dataset.from_dict({"idx": list(range(N_DOCS)), "question": questions})
            self.dataset = datasets.DatasetDict({"test": ds})
            self.dataset_no_image = self.dataset

    seen = []

    def process_results(doc, results):
        seen.append([doc["idx"], results[0]])
        return {"exact": 1.0}

    cfg = dict(task="tiny_vdc", dataset_path="in-memory", test_split="test", output_type="generate_until",
               doc_to_visual=lambda doc: [frames[doc["idx"]]], doc_to_text=lambda doc, kw=None: doc["question"], doc_to_target="idx",
               generation_kwargs={"max_new_tokens": 8, "temperature": 0, "do_sample": False},
               process_results=process_results,
               metric_list=[{"metric": "exact", "aggregation": lambda xs: sum(xs) / len(xs), "higher_is_better": True}])
    t = InMemoryCaptionTask(config=cfg, model_name="auroracap_mi355x")
    lm.task_dict = {"tiny_vdc": {"test": t.dataset["test"]}}                          # what evaluator.simple_evaluate hands the model
    res = evaluator.evaluate(lm=lm, task_dict={"tiny_vdc": t}, limit=None, bootstrap_iters=0, log_samples=True)
    assert res is not None and sorted(i for i, _ in seen) == list(range(N_DOCS))
    rec = {"model_args": MODEL_ARGS, "additional_config": json.dumps(ADDITIONAL), "init_kwargs": json.dumps(init_kwargs, sort_keys=True),
           "generate_until_calls": json.dumps(calls), "responses_by_doc": json.dumps(seen),
           "note": "requests: [context, gen_kwargs, doc_id, task, split] (doc_to_visual = [frames of that document]); docs: "
                   "tests/golden/make_golden_harness.py docs()"}
    np.savez_compressed(os.path.join(HERE, "g16_lmms_harness.npz"), **rec)
    print(json.dumps({k: v for k, v in rec.items() if k != "note"}, indent=1)[:3000])


if __name__ == "__main__":
    main()

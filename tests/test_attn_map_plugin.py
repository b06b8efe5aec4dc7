"""The lmms-eval adaptor with attn_map=True: every response gets `visual_share` - per generated token, the share of its attention that
went to the visual tokens - in `extras`, in both the chunked and the streaming mode; off, nothing is asked of the model."""
from types import SimpleNamespace

import numpy as np
import pytest

from aurora_amd.lmms_plugin.models import auroracap_mi355x as P
from tests.test_lmms_plugin import FakeModel, FakeTok, fake_pre


def result(px, ids):
    out = [int(px.shape[0]), len(ids)]
    return dict(ids=out, attn_map=np.zeros((2, 64), np.float32), visual_share=np.array([0.0, px.shape[0] / 8], np.float32))


class Recording(FakeModel):
    def caption_batch(self, clips, max_new_tokens=2048, attn_map=None):
        self.calls.append(attn_map)
        return [result(px, ids) if attn_map is not None else [int(px.shape[0]), len(ids)] for px, ids in clips]


class Streaming(Recording):
    def caption_stream(self, clips, max_new_tokens=2048, on_error=None, attn_map=None):
        self.calls.append(attn_map)
        for k, (px, ids) in enumerate(clips):
            yield k, (result(px, ids) if attn_map is not None else [int(px.shape[0]), len(ids)])


def requests(m, n=5):
    m.task_dict = {"vdc": {"test": {i: np.zeros((2 + i % 3, 8, 8, 3), np.uint8) for i in range(n)}}}
    return [SimpleNamespace(args=("q" * (1 + i), {}, lambda d: [d], i, "vdc", "test")) for i in range(n)]


@pytest.mark.parametrize("model", [Recording, Streaming])
def test_visual_share_reaches_the_extras_of_its_own_request(model):
    make = lambda **kw: P.AuroraCapMI355X(pretrained="unused", device="cpu", batch_size=2, _model=model(), _tokenizer=FakeTok(),   # noqa: E731
                                          _preprocessor=fake_pre, **kw)
    off = make()
    plain = off.generate_until(requests(off))
    assert off.extras == {} and set(off.model.calls) == {None}
    on = make(attn_map="true")
    assert on.attn_map is True
    assert on.generate_until(requests(on)) == plain
    assert set(map(repr, on.model.calls)) == {repr(dict(keys=None))}
    assert sorted(on.extras) == list(range(5))
    for i in range(5):
        assert on.extras[i] == dict(visual_share=[0.0, (2 + i % 3) / 8])
    with pytest.raises(NotImplementedError):
        sf = make(attn_map=True, slowfast=True)
        sf.generate_until(requests(sf))

"""Python operator seam of the reference, re-hosted on the MI355X engine (drop-in for this path only).

The three calls every reference caller makes (inference.py:87-96, gradio_gui.py:83-92,
lmms_eval/models/auroracap.py:500-509):

    model.visual_encoder.reset_tome_r(token_kept_ratio)
    output = model(data, mode="inference")            # data: {"pixel_values", "input_ids"}
    cont = model.llm.generate(**output, do_sample=False, temperature=0.0, top_p=1.0, num_beams=1,
                              max_new_tokens=N)       # LongTensor [1, <= N]: new ids only

keep their names, argument meaning and error behaviour (NotImplementedError for unknown modes,
aurora.py:269-270).  Decoding is greedy (`do_sample=False`, what inference.py:91 hard-codes) or seeded sampling
(`do_sample=True`: temperature / top-k / top-p as aurora_amd.sampling defines them); beam search does not exist on this path.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .engine import AuroraCapEngine, splice_rows, tokens_at_layer
from .logit_rules import KEYS as LOGIT_RULE_KEYS, check_logit_rules
from . import guidance as GD
from .guidance import pair_slots
from . import stopping as ST
from .sampling import DEFAULT_TOP_K, check_sampling
from .scoring import check_logprobs
from . import attn_map as AM

DEFAULT_IMAGE_TOKEN = "<image>"          # src/xtuner/xtuner/utils/constants.py:5
IMAGE_TOKEN_INDEX = -200                 # constants.py:4
VICUNA_INSTRUCTION = "USER: {input} ASSISTANT:"   # utils/templates.py:92 (PROMPT_TEMPLATE.vicuna)


def process_text(inputs: str, tokenizer) -> torch.Tensor:
    """inference.py:12-27: split on <image>, BOS only on the first chunk, -200 between chunks -> [1, n] ids."""
    ids = []
    chunks = inputs.split(DEFAULT_IMAGE_TOKEN)
    for idx, chunk in enumerate(chunks):
        enc = tokenizer.encode(chunk) if idx == 0 else tokenizer.encode(chunk, add_special_tokens=False)
        ids.extend(enc)
        if idx != len(chunks) - 1:
            ids.append(IMAGE_TOKEN_INDEX)
    return torch.tensor(ids).unsqueeze(0)


def build_prompt(prompt: str, num_images: int) -> str:
    """inference.py:76-85."""
    return VICUNA_INSTRUCTION.format(input=" ".join([DEFAULT_IMAGE_TOKEN] * num_images) + "\n" + prompt, round=1)


def generation_top_k(path: str) -> Optional[int]:
    """`top_k` of the language model's generation_config.json under an xtuner-layout checkpoint directory, or None."""
    import json
    import os
    for sub in ("llm", ""):
        f = os.path.join(path, sub, "generation_config.json")
        if os.path.isfile(f):
            with open(f) as fh:
                k = json.load(fh).get("top_k")
            return None if k is None else int(k)
    return None


def generation_logit_rules(path: str) -> dict:
    """The `repetition_penalty` / `no_repeat_ngram_size` / `min_new_tokens` the language model's generation_config.json sets under an
    xtuner-layout checkpoint directory (found the way `generation_top_k` finds it): only the keys it holds with a value, {} without."""
    import json
    import os
    for sub in ("llm", ""):
        f = os.path.join(path, sub, "generation_config.json")
        if os.path.isfile(f):
            with open(f) as fh:
                cfg = json.load(fh)
            return {k: cfg[k] for k in LOGIT_RULE_KEYS if cfg.get(k) is not None}
    return {}


class AuroraEncoder:
    """visual_encoder handle (aurora.py:869-904): only the ratio knob and the r formula live on the host."""

    def __init__(self, engine: AuroraCapEngine, visual_token_merge_ratio: float = 1.0):
        self._e = engine
        self.visual_token_merge_ratio = visual_token_merge_ratio
        self.config = engine.v

    def reset_tome_r(self, visual_token_merge_ratio: float):            # aurora.py:880-881
        self.visual_token_merge_ratio = visual_token_merge_ratio

    def __call__(self, pixel_values: torch.Tensor, output_merge_map: bool = False):
        """tokens [F, n_kept, D]; output_merge_map=True: (tokens, map int32 [F, gh, gw], sizes fp32 [F, n_kept]) - which token
        every patch was merged into and how many patches each token holds (`aurora_amd.merge_map`)."""
        r = self._e.tome_r(self.visual_token_merge_ratio, pixel_values.shape[-2], pixel_values.shape[-1])
        return self._e.vit_encode(pixel_values, r, merge_map=output_merge_map)


class GenerateOutput:
    """What `_LLM.generate(return_dict_in_generate=True)` returns: `sequences` LongTensor [1, n] (what the plain call returns) and,
    with output_logprobs=True, `token_logprobs` float32 [1, n], `top_ids` long [1, n, k], `top_logprobs` float32 [1, n, k]
    (k = top_logprobs; `aurora_amd.scoring.token_logprobs` is the definition) - else None.  With output_attentions=True,
    `prompt_attention` float32 [1, n, W]: row i the attention of the step that picked token i over keys [0, W) of its context, mean
    over layers and heads (`aurora_amd.attn_map`; row 0, the prefill's token, is zeros); and, when the visual rows were passed
    (`vis_rows`, what `AuroraModel.forward` adds with data["output_attentions"]), `visual_attention` float32 [n, nvis] - its columns at
    the visual tokens - and `visual_share` float32 [n], its row sums: how much of each token's attention went to the visual prefix."""

    def __init__(self, sequences, token_logprobs=None, top_ids=None, top_logprobs=None, prompt_attention=None, visual_attention=None,
                 visual_share=None):
        self.sequences, self.token_logprobs, self.top_ids, self.top_logprobs = sequences, token_logprobs, top_ids, top_logprobs
        self.prompt_attention, self.visual_attention, self.visual_share = prompt_attention, visual_attention, visual_share


def split_stop_arguments(eos_token_id, stop_strings=None, stop_token_ids=None):
    """transformers' keywords -> (the batch's EOS, a `stop=` dict or None): eos_token_id may be a list, whose first id is the EOS and
    whose other ids are stop ids, in front of stop_token_ids; stop_strings may be one string."""
    ids = []
    if isinstance(eos_token_id, (list, tuple)):
        eos_token_id, ids = (eos_token_id[0], list(eos_token_id[1:])) if len(eos_token_id) else (None, [])
    ids += [] if stop_token_ids is None else list(stop_token_ids)
    strings = [] if stop_strings is None else ([stop_strings] if isinstance(stop_strings, str) else list(stop_strings))
    ids = [t for k, t in enumerate(ids) if t != eos_token_id and t not in ids[:k]]       # the EOS already stops; duplicates say nothing new
    if not ids and not strings:
        return eos_token_id, None
    return eos_token_id, dict(token_ids=ids, strings=strings)


class _LLM:
    def __init__(self, engine: AuroraCapEngine, eos_token_id: Optional[int]):
        self._e = engine
        self.eos_token_id = eos_token_id
        self.generation_top_k = None          # generation_config.json's top_k, when the checkpoint has one (AuroraModel.from_pretrained)
        self.generation_logit_rules = {}      # its repetition_penalty / no_repeat_ngram_size / min_new_tokens, those it sets
        self.config = engine.l
        self._stop_tokenizer = None           # the tokenizer whose byte table the engine holds (use_tokenizer)

    def use_tokenizer(self, tokenizer):
        """Stop strings are matched on the bytes the tokens decode to: build the tokenizer's table (`stopping.token_bytes`) and hand
        it to the engine, once per tokenizer."""
        if tokenizer is not self._stop_tokenizer:
            self._e.set_stop_vocab(ST.token_bytes(tokenizer, self.config.get("vocab_size")))
            self._stop_tokenizer = tokenizer

    def generate(self, inputs_embeds: torch.Tensor = None, do_sample: bool = False, temperature: float = 0.0, top_p: float = 1.0,
                 num_beams: int = 1, max_new_tokens: int = 2048, input_ids=None, position_ids=None, attention_mask=None,
                 past_key_values=None, labels=None, eos_token_id="default", top_k="default", seed: int = 0, stream: int = 0,
                 output_logprobs: bool = False, top_logprobs: int = 0, return_dict_in_generate: bool = False,
                 repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                 min_new_tokens: Optional[int] = None, stop_strings=None, tokenizer=None, stop_token_ids=None, merge_map=None,
                 merge_sizes=None, output_attentions: bool = False, attention_keys: Optional[int] = None, attention_layers=None,
                 vis_rows=None, guidance_scale: Optional[float] = None, negative_prompt_ids=None, negative_inputs_embeds=None, **unused):
        """`merge_map` / `merge_sizes` (what `AuroraModel.forward` adds with data["output_merge_map"]) are accepted and ignored, so
        `generate(**out, ...)` keeps working.
        output_attentions=True (transformers' flag; needs return_dict_in_generate=True, ValueError otherwise): the result carries
        `prompt_attention` [1, n, W] - W = attention_keys, a multiple of 64, or the prompt length rounded up to 64 -, averaged over
        attention_layers (None = all) and all heads, and with `vis_rows` also `visual_attention` / `visual_share`.  The ids are
        the same.
        do_sample=False: greedy; `temperature` / `top_p` are ignored, as transformers ignores them.  do_sample=True: seeded
        sampling with `temperature` (> 0), `top_p` and `top_k`.  The default temperature stays 0.0 (what every reference caller
        passes for greedy), not transformers' 1.0, so do_sample=True without a temperature raises ValueError: pass one.  The
        ids are a function of (seed, stream) and the prompt alone.
        top_k follows the transformers range the reference pins (<= 4.42), whose GenerationConfig defaults it to 50 - later
        releases report None -; a `top_k` in the checkpoint's generation_config.json (`self.generation_top_k`) wins over that default,
        an explicit argument over both; top_k=0 turns the filter off.
        return_dict_in_generate=True: a `GenerateOutput` instead of the ids tensor; with output_logprobs=True it carries the
        log-probability of every generated token and its `top_logprobs` (0 .. 8) most likely alternatives, under the model's
        unmodified distribution whatever do_sample says.  output_logprobs=True needs return_dict_in_generate=True (ValueError);
        `output_scores` stays ignored.
        repetition_penalty (1.0 = off), no_repeat_ngram_size (0 = off), min_new_tokens (0 = off): transformers' three logits
        processors on the raw row ahead of the pick, greedy or sampled (`aurora_amd.logit_rules`).  Their history is the tokens
        GENERATED so far, not the prompt - what transformers sees here too, since `generate(inputs_embeds=...)` starts `input_ids`
        empty.  None (the default): the value of the checkpoint's generation_config.json (`self.generation_logit_rules`) when it
        sets one, else off; an explicit argument wins.  Values transformers rejects raise ValueError.  Log-probabilities stay
        those of the unmodified row.
        stop_strings=[...] with tokenizer=tok (transformers requires the tokenizer too; without it: ValueError): generation ends
        behind the token whose text completes one of the strings, which stays in the output, as with transformers'
        StopStringCriteria (`aurora_amd.stopping`).  eos_token_id may be a list: its first id is the EOS, the others - and
        stop_token_ids - end the generation the same way, but `min_new_tokens` holds back the first alone.
        guidance_scale (None or 1 = off) with negative_prompt_ids (text ids, [n] or [1, n], through the embedding table) or
        negative_inputs_embeds ([1, n, d]): transformers' classifier-free guidance (`aurora_amd.guidance`), the first processor ahead
        of the three above - every pick contrasts the prompt's distribution with the negative prompt's, which decodes in a second
        KV slot (an engine with max_batch >= 2).  transformers falls back to the prompt's last token when no negative is given; with
        inputs_embeds there is none, so a scale without a negative raises ValueError.  Log-probabilities stay those of the model's
        conditional row."""
        gscale = GD.check_scale(guidance_scale)
        if gscale is not None and negative_prompt_ids is None and negative_inputs_embeds is None:
            raise ValueError("guidance_scale needs negative_prompt_ids or negative_inputs_embeds: the prompt is embeddings, so there is no default negative prompt")
        if stop_strings is not None and tokenizer is None:
            raise ValueError("stop_strings needs tokenizer= as well: the strings are matched on the text the tokens decode to")
        if output_logprobs and not return_dict_in_generate:
            raise ValueError("output_logprobs=True needs return_dict_in_generate=True (the plain call returns the ids tensor alone)")
        if output_attentions and not return_dict_in_generate:
            raise ValueError("output_attentions=True needs return_dict_in_generate=True (the plain call returns the ids tensor alone)")
        lpn = check_logprobs(top_logprobs) if output_logprobs else None
        am = dict(keys=attention_keys, layers=attention_layers) if output_attentions else None
        if am is not None:
            AM.check_attn_map(am, self.config["num_hidden_layers"])
        if inputs_embeds is None:
            raise ValueError("generate() on this path takes inputs_embeds (the output of model(data, mode='inference'))")
        if num_beams != 1:
            raise NotImplementedError("beam search is not implemented on the MI355X path (num_beams=1 only)")
        sampling = None
        if do_sample:
            if top_k == "default":
                top_k = DEFAULT_TOP_K if self.generation_top_k is None else self.generation_top_k
            sampling = check_sampling(dict(temperature=temperature, top_p=top_p, top_k=top_k, seed=seed))
        given = dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens)
        rules = check_logit_rules({k: self.generation_logit_rules.get(k) if v is None else v for k, v in given.items()})
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[0] != 1:
            raise ValueError(f"inputs_embeds must be [1, L, {self.config['hidden_size']}], got {tuple(inputs_embeds.shape)}")
        eos = self.eos_token_id if eos_token_id == "default" else eos_token_id
        eos, stop = split_stop_arguments(eos, stop_strings, stop_token_ids)
        if stop is not None and stop.get("strings"):
            self.use_tokenizer(tokenizer)
        L, d = inputs_embeds.shape[1], inputs_embeds.shape[2]
        pad = torch.zeros((L + 31) // 32 * 32, d, dtype=torch.float16, device=self._e.dev)
        pad[:L] = inputs_embeds[0].to(device=self._e.dev, dtype=torch.float16)
        n = min(max_new_tokens, self._e.max_new_tokens)
        kw = dict(sampling=sampling, streams=[stream]) if sampling else {}
        if rules is not None:
            kw["logit_rules"] = rules
        if stop is not None:
            kw["stop"] = stop
        if am is not None:
            kw["attn_map"] = am
        if gscale is not None:
            if negative_inputs_embeds is not None:
                ne = negative_inputs_embeds
                if ne.dim() != 3 or ne.shape[0] != 1 or ne.shape[2] != d or ne.shape[1] < 1:
                    raise ValueError(f"negative_inputs_embeds must be [1, n, {d}], got {tuple(ne.shape)}")
                Ln = ne.shape[1]
                npad = torch.zeros((Ln + 31) // 32 * 32, d, dtype=torch.float16, device=self._e.dev)
                npad[:Ln] = ne[0].to(device=self._e.dev, dtype=torch.float16)
            else:
                nids = negative_prompt_ids.reshape(-1).tolist() if torch.is_tensor(negative_prompt_ids) else [int(t) for t in np.asarray(negative_prompt_ids).reshape(-1)]
                npad, Ln = self._e.text_embeds(nids)
            kw["guidance"] = dict(scale=gscale, negative=[(npad, Ln)])
        if lpn is None and am is None:
            ids = self._e.generate([pad], [L], n, eos_id=eos, **kw)[0]
            seq = torch.tensor([ids], dtype=torch.long)
            return GenerateOutput(seq) if return_dict_in_generate else seq
        r = self._e.generate([pad], [L], n, eos_id=eos, **({} if lpn is None else dict(logprobs=lpn)), **kw)[0]
        out = GenerateOutput(torch.tensor([r["ids"]], dtype=torch.long))
        if lpn is not None:
            out.token_logprobs, out.top_logprobs = torch.from_numpy(r["token_logprobs"]).unsqueeze(0), torch.from_numpy(r["top_logprobs"]).unsqueeze(0)
            out.top_ids = torch.from_numpy(r["top_ids"].astype("int64")).unsqueeze(0)
        if am is not None:
            out.prompt_attention = torch.from_numpy(r["attn_map"]).unsqueeze(0)
            if vis_rows is not None:
                rows = vis_rows.cpu().numpy() if torch.is_tensor(vis_rows) else vis_rows
                va = AM.visual(r["attn_map"], rows)
                out.visual_attention, out.visual_share = torch.from_numpy(va), torch.from_numpy(va.sum(1, dtype=va.dtype))
        return out


class AuroraModel:
    def __init__(self, engine: AuroraCapEngine, eos_token_id: Optional[int] = 2, slowfast: bool = False):
        self.engine = engine
        self.slowfast = slowfast                                                  # aurora.py:81 (AuroraModel(slowfast=...))
        self.visual_encoder = AuroraEncoder(engine)
        self.llm = _LLM(engine, eos_token_id)

    @classmethod
    def from_pretrained(cls, path: str, *, max_frames: int = 16, max_ctx: int = 8192, max_new_tokens: int = 2048,
                        max_batch: int = 1, slowfast: bool = False, **kw):
        from .checkpoint import load_auroracap
        cfg, weights = load_auroracap(path)
        eng = AuroraCapEngine(cfg, weights, max_frames=max_frames, max_batch=max_batch, max_ctx=max_ctx,
                              max_new_tokens=max_new_tokens, **kw)
        model = cls(eng, cfg["llm"].get("eos_token_id", 2), slowfast=slowfast)
        model.llm.generation_top_k = generation_top_k(path)
        model.llm.generation_logit_rules = generation_logit_rules(path)
        return model

    def caption_batch(self, clips, max_new_tokens: int = 2048, eos_token_id="default", sampling=None, streams=None, share=None,
                      logprobs: Optional[int] = None, logit_rules: Optional[dict] = None, stop=None, attn_map: Optional[dict] = None,
                      guidance_scale: Optional[float] = None, negative_prompt=None, tokenizer=None):
        """Several clips through the three calls at once (what a harness gets by looping inference.py:87-96 over its
        requests): clips = [(pixel_values [f, c, h, w], input_ids with -200 markers), ...] -> list of new-token id lists,
        identical per clip to the one-at-a-time calls.  Uses visual_encoder.visual_token_merge_ratio.
        sampling=dict(temperature, top_k, top_p, seed): sampled captions, clip i drawing with stream streams[i] (default: i).
        share: one hashable key per clip (or None); clips of equal key are the same visual input and share its ViT pass and the KV
        of their common prefix inside a chunk of max_batch clips (AuroraCapEngine.caption_batch).
        logprobs=n (0 .. 8): a dict per clip instead - ids, token_logprobs, top_ids, top_logprobs (AuroraCapEngine.generate).
        logit_rules=dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0): the three rules of `llm.generate` for
        every clip of the call, each over its own generated tokens (not its prompt).
        stop=dict(token_ids=(), strings=(), max_new_tokens=0) for every clip, or a list with one dict or None per clip: stop ids,
        stop strings (`llm.use_tokenizer(tok)` first) and a budget of the clip's own (AuroraCapEngine.generate).
        attn_map=dict(keys=W or None, layers=None or a list): a dict per clip that also holds attn_map float32 [n, W]
        (AuroraCapEngine.generate), visual_attention [n, nvis] - its columns at the clip's visual tokens - and visual_share [n].
        guidance_scale (None or 1 = off): classifier-free guidance for every clip (AuroraCapEngine.caption_batch); negative_prompt
        None: each clip's own prompt without its frames; a text (with tokenizer=, or the one `llm.use_tokenizer` got) or its input
        ids: that prompt for every clip.  A chunk then holds max_batch // 2 clips."""
        gd = self._guidance(guidance_scale, negative_prompt, tokenizer)
        check_logprobs(logprobs)
        if attn_map is not None:
            AM.check_attn_map(attn_map, self.llm.config["num_hidden_layers"])
        rules = check_logit_rules(logit_rules)
        eos = self.llm.eos_token_id if eos_token_id == "default" else eos_token_id
        out = []
        B = self.engine.max_batch
        if gd is not None:
            pair_slots(1, B)
            B //= 2
        n = min(max_new_tokens, self.engine.max_new_tokens)
        if stop is not None and not isinstance(stop, dict):
            stop = list(stop)
            if len(stop) != len(clips):
                raise ValueError(f"{len(stop)} stop records for {len(clips)} clips")
        for c0 in range(0, len(clips), B):
            group = [(px, ids.tolist() if torch.is_tensor(ids) else list(ids)) for px, ids in clips[c0:c0 + B]]
            st = range(c0, c0 + len(group)) if streams is None else list(streams)[c0:c0 + len(group)]
            kw = dict(sampling=sampling, streams=st) if sampling is not None else {}
            if share is not None:
                kw["share"] = list(share)[c0:c0 + len(group)]
            if logprobs is not None:
                kw["logprobs"] = logprobs
            if rules is not None:
                kw["logit_rules"] = rules
            if stop is not None:
                kw["stop"] = stop if isinstance(stop, dict) else stop[c0:c0 + len(group)]
            if attn_map is not None:
                kw["attn_map"] = attn_map
            if gd is not None:
                kw["guidance"] = gd
            res = self.engine.caption_batch(group, self.visual_encoder.visual_token_merge_ratio, n, eos, **kw)
            if attn_map is not None:
                for (px, ids), r in zip(group, res):
                    self._add_visual(r, px.shape, ids)
            out.extend(res)
        return out

    def _guidance(self, guidance_scale, negative_prompt, tokenizer=None) -> Optional[dict]:
        """guidance_scale / negative_prompt of a caption call -> the engine's `guidance=` dict, or None (no request)"""
        g = GD.check_scale(guidance_scale)
        if g is None:
            return None
        if self.slowfast:
            raise NotImplementedError("guidance on a slow-fast model (ragged per-frame token counts)")
        if isinstance(negative_prompt, str):
            tok = tokenizer if tokenizer is not None else self.llm._stop_tokenizer
            if tok is None:
                raise ValueError("negative_prompt as text needs tokenizer= (or llm.use_tokenizer(tok) earlier); pass its input ids otherwise")
            negative_prompt = tok(negative_prompt).input_ids
        if negative_prompt is not None:
            negative_prompt = negative_prompt.reshape(-1).tolist() if torch.is_tensor(negative_prompt) else [int(t) for t in negative_prompt]
        return dict(scale=g, negative_ids=negative_prompt)

    def _add_visual(self, r: dict, shape, ids):
        """visual_attention [n, nvis] and visual_share [n] beside a result's attn_map: its columns at the context positions of the
        clip's visual tokens under the current merge ratio (the splice plan's vis_rows), and their row sums"""
        e = self.engine
        tr = e.tome_r(self.visual_encoder.visual_token_merge_ratio, shape[-2], shape[-1])
        t0 = (shape[-2] // e.v["patch_size"]) * (shape[-1] // e.v["patch_size"]) + 1
        rows = splice_rows(ids, shape[0], tokens_at_layer(t0, tr, e.v["num_hidden_layers"] - 1) - 1)["vis_rows"]
        r["visual_attention"] = AM.visual(r["attn_map"], rows)
        r["visual_share"] = r["visual_attention"].sum(1, dtype=np.float32)

    def loglikelihood_batch(self, items, share: bool = True):
        """Log-likelihood of given continuations: items = [(pixel_values [f, c, h, w], context ids with -200 markers, continuation
        ids)] -> per item dict(logprob, greedy, token_logprobs, count), in order (AuroraCapEngine.loglikelihood_batch; it cuts
        the items into chunks of max_batch itself).  Uses visual_encoder.visual_token_merge_ratio.  A slow-fast model raises."""
        if self.slowfast:
            raise NotImplementedError("loglikelihood_batch on a slow-fast model (ragged per-frame token counts)")
        as_list = lambda ids: ids.tolist() if torch.is_tensor(ids) else list(ids)      # noqa: E731
        return self.engine.loglikelihood_batch([(px, as_list(c), as_list(t)) for px, c, t in items],
                                               self.visual_encoder.visual_token_merge_ratio, share=share)

    def caption_prompts(self, pixel_values, list_of_input_ids, max_new_tokens: int = 2048, eos_token_id="default", sampling=None,
                        streams=None, logit_rules: Optional[dict] = None, stop=None, guidance_scale: Optional[float] = None,
                        negative_prompt=None, tokenizer=None):
        """One clip, several prompts (the five VDC questions about a video): pixel_values [f, c, h, w], each prompt's input ids with
        -200 markers -> one new-token id list per prompt, in order, each identical to captioning (clip, prompt) alone.  The ViT runs
        once per chunk of max_batch prompts and the later prompts prefill only the rows behind the last visual token.  A slow-fast
        model never shares: its prompts run one at a time through the three calls.  logit_rules / stop: as in `caption_batch`
        (a slow-fast model takes no stop records).  guidance_scale / negative_prompt / tokenizer: as in `caption_batch`; the ViT
        still runs once per chunk, the prompts' KV is not shared."""
        rules = check_logit_rules(logit_rules)
        self._guidance(guidance_scale, negative_prompt, tokenizer)
        prompts = [ids.tolist() if torch.is_tensor(ids) else list(ids) for ids in list_of_input_ids]
        if self.slowfast and stop is not None:
            raise NotImplementedError("caption_prompts(stop=) on a slow-fast model")
        if self.slowfast:
            out, ratio = [], self.visual_encoder.visual_token_merge_ratio
            for k, ids in enumerate(prompts):
                self.visual_encoder.reset_tome_r(ratio)                           # the slow-fast forward leaves it at 1.0
                emb = self.forward({"pixel_values": pixel_values.unsqueeze(0), "input_ids": [ids]}, mode="inference")
                kw = dict(do_sample=False) if sampling is None else dict(sampling, do_sample=True, stream=k if streams is None else list(streams)[k])
                kw.update(rules if rules is not None else dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0))
                out.append(self.llm.generate(**emb, num_beams=1, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id, **kw)[0].tolist())
            self.visual_encoder.reset_tome_r(ratio)
            return out
        return self.caption_batch([(pixel_values, ids) for ids in prompts], max_new_tokens, eos_token_id, sampling, streams,
                                  share=[0] * len(prompts), **({} if rules is None else dict(logit_rules=rules)),
                                  **({} if stop is None else dict(stop=stop)),
                                  **({} if guidance_scale is None else dict(guidance_scale=guidance_scale, negative_prompt=negative_prompt, tokenizer=tokenizer)))

    def caption_stream(self, clips, max_new_tokens: int = 2048, eos_token_id="default", check_every: int = 16, on_error=None,
                       overlap=None, sampling=None, stream_of=None, share_key=None, logit_rules: Optional[dict] = None, stop=None,
                       attn_map: Optional[dict] = None):
        """Continuous batching over an iterable of (pixel_values, input_ids): yields (index, new-token ids) as captions
        finish (EOS or max_new_tokens), re-filling freed KV slots with the next clips.  Per-clip results equal the
        one-at-a-time calls.  overlap (default: on for an engine with spare KV sequences): the next clips' front ends run
        ahead on a CU-masked stream while the slots decode (AuroraCapEngine.caption_stream).
        sampling=dict(temperature, top_k, top_p, seed): sampled captions; clip k draws with stream stream_of(k) (default: k).
        share_key: callable index -> key | None; clips of equal key are the same visual input (engine built with prefix_cache >= 1).
        logit_rules: as in `caption_batch`; a clip's history starts empty in whatever slot it lands.
        stop: one dict for every clip, or a callable index -> dict | None (AuroraCapEngine.caption_stream): a clip with a budget of
        its own gives its slot back when it is reached.
        attn_map: as in `caption_batch` - yields (index, dict) with attn_map, visual_attention and visual_share."""
        rules = check_logit_rules(logit_rules)
        if attn_map is not None:
            AM.check_attn_map(attn_map, self.llm.config["num_hidden_layers"])
        eos = self.llm.eos_token_id if eos_token_id == "default" else eos_token_id
        n = min(max_new_tokens, self.engine.max_new_tokens)
        seen = {}                                                                 # index -> (pixel shape, ids) of the clips in flight (attn_map)

        def it():
            for k, (px, ids) in enumerate(clips):
                ids = ids.tolist() if torch.is_tensor(ids) else list(ids)
                if attn_map is not None:
                    seen[k] = (tuple(px.shape), ids)
                yield px, ids
        for k, r in self.engine.caption_stream(it(), self.visual_encoder.visual_token_merge_ratio, n, eos, check_every=check_every,
                                               on_error=on_error, overlap=overlap,
                                               **(dict(share_key=share_key) if share_key is not None else {}),
                                               **(dict(sampling=sampling, stream_of=stream_of) if sampling is not None else {}),
                                               **(dict(logit_rules=rules) if rules is not None else {}),
                                               **(dict(stop=stop) if stop is not None else {}),
                                               **(dict(attn_map=attn_map) if attn_map is not None else {})):
            if attn_map is not None:
                self._add_visual(r, *seen.pop(k))
            yield k, r

    def __call__(self, data: dict, data_samples=None, mode: str = "loss"):
        return self.forward(data, data_samples, mode)

    def forward(self, data: dict, data_samples=None, mode: str = "loss"):
        if mode != "inference":
            # aurora.py:261-270: 'loss' / 'predict' / 'tensor' are training-side modes, anything else raises
            raise NotImplementedError(f"mode={mode!r}: only mode='inference' exists on the MI355X path")
        if "pixel_values" not in data:
            raise KeyError("data['pixel_values'] is required")
        px = data["pixel_values"]
        if px.dim() == 4:                                   # single image -> one-frame video (aurora.py:217-218)
            px = px.unsqueeze(1)
        if px.dim() != 5 or px.shape[0] != 1:
            raise ValueError(f"pixel_values must be [1, f, c, h, w] or [1, c, h, w], got {tuple(data['pixel_values'].shape)}")
        ids = data["input_ids"]
        ids = ids[0].tolist() if torch.is_tensor(ids) else list(ids[0])
        want_map = bool(data.get("output_merge_map"))
        want_rows = bool(data.get("output_attentions"))         # the context positions of the visual tokens, for `llm.generate(vis_rows=...)`
        vis_rows = None
        maps = None
        enc = (lambda p: self.visual_encoder(p, output_merge_map=True)) if want_map else self.visual_encoder
        if self.slowfast and px.shape[1] != 1:                                    # aurora.py:223-246
            low = enc(px[0, 1:])                                                  # frames 1.. at the current ratio
            self.visual_encoder.visual_token_merge_ratio = 1.0                    # :231 - the reference leaves it at 1.0 too
            high = enc(px[0, :1])                                                 # frame 0 unmerged
            if want_map:                                                          # frame 0 carries the identity map and ones
                (low, lmap, lsz), (high, hmap, hsz) = low, high
                maps = (torch.cat([hmap, lmap], 0), [hsz[0]] + list(lsz))
            flat = torch.cat([high.reshape(-1, high.shape[-1]), low.reshape(-1, low.shape[-1])], 0)
            counts = [high.shape[1]] + [low.shape[1]] * low.shape[0]
            plan = self.engine.splice_plan(ids, px.shape[1], counts, strict=True)  # utils.py:297-431: marker i <- frame i
            embeds, L = self.engine.project_splice(flat, plan=plan)
            if want_rows:
                vis_rows = splice_rows(ids, px.shape[1], counts, strict=True)["vis_rows"]
        else:
            vis = enc(px[0])                                                      # aurora.py:249-253
            if want_map:
                vis, vmap, vsz = vis
                maps = (vmap, list(vsz))
            embeds, L = self.engine.project_splice(vis, ids)                     # aurora.py:254-258
            if want_rows:
                vis_rows = splice_rows(ids, vis.shape[0], vis.shape[1])["vis_rows"]
        out = {"input_ids": None, "position_ids": None, "attention_mask": None, "past_key_values": None,
               "inputs_embeds": embeds[:L].unsqueeze(0), "labels": None}          # utils.py:288-295
        if want_map:                      # merge_map int32 [f, gh, gw], merge_sizes: f tensors fp32 [tokens of that frame] (merge_map.py)
            out["merge_map"], out["merge_sizes"] = maps
        if want_rows:
            out["vis_rows"] = torch.from_numpy(vis_rows)
        return out

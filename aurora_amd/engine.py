"""Host side of the MI355X AuroraCap path: owns torch-allocated device memory (weights, workspace, KV
pool), re-lays weights into the kernels' fragment format once, and drives libaurora_hip.so through its
C ABI.  PyTorch is used for memory / stream housekeeping only - no torch compute op is on the hot path.

Weight dictionaries use the reference checkpoints' parameter names (HF CLIP vision tower, xtuner
projector `model.0 / model.2`, HF Llama), grouped as
    {"vit": {...,"layers":[{...}]}, "projector": {...}, "llm": {...,"layers":[{...}]}}
exactly like `oracle/aurora_oracle.py` consumes them, so parity tests feed both sides the same tensors.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import guidance as GD
from . import logit_rules as LR
from . import stopping as ST
from . import sampling as S
from .scoring import check_logprobs
from . import attn_map as AM
from ._lib import AurConfig, check

IMAGE_TOKEN_INDEX = -200     # src/xtuner/xtuner/utils/constants.py:4


def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def tome_r(height: int, width: int, patch: int, token_kept_ratio: float, num_layers: int) -> int:
    """aurora.py:895 (evaluated inside the C library in doubles, same operation order)."""
    return int(_lib.lib().aur_tome_r(height, width, patch, float(token_kept_ratio), num_layers))


def tokens_at_layer(t0: int, r: int, layer: int) -> int:
    return int(_lib.lib().aur_tokens_at_layer(t0, r, layer))


def projector_settings(pc: dict, visual_hidden: Optional[int], llm_hidden: Optional[int]) -> dict:
    """Validated ProjectorConfig values (configuration_projector.py:9-22; defaults = the class's own: depth 2, 'gelu', bias True).
    Raises on what the kernels do not implement instead of loading it wrong."""
    depth, act, bias = int(pc.get("depth", 2)), pc.get("hidden_act", "gelu"), bool(pc.get("bias", True))
    if not 1 <= depth <= 8:
        raise NotImplementedError(f"projector depth {depth}: 1 .. 8 Linear layers are supported")
    if act not in _lib.ACT_BY_NAME:
        raise NotImplementedError(f"projector hidden_act {act!r}: the GEMM epilogues implement {sorted(_lib.ACT_BY_NAME)}")
    for key, have in (("visual_hidden_size", visual_hidden), ("llm_hidden_size", llm_hidden)):
        if key in pc and have is not None and int(pc[key]) != int(have):
            raise ValueError(f"projector config {key} = {pc[key]} but the {'vision tower' if key[0] == 'v' else 'language model'} has hidden size {have}")
    return dict(depth=depth, hidden_act=act, bias=bias)


PROMPT_BUCKETS = (0, 32, 64, 128)


def check_prompt_bucket(bucket: int) -> int:
    """0 = every prompt is laid out at its exact length; 32 / 64 / 128 = at the next multiple of the bucket (`prompt_stride`)."""
    if bucket not in PROMPT_BUCKETS:
        raise ValueError(f"prompt_bucket {bucket!r} is not one of {PROMPT_BUCKETS}")
    return int(bucket)


def prompt_stride(seq_len: int, bucket: int) -> int:
    """Rows between the sequences of a prefill pass that holds a prompt of `seq_len` positions; bucket 0: the exact length (the
    equal-length entry points pad it to a multiple of 32 themselves)."""
    return _rup(seq_len, bucket) if bucket else seq_len


def prefill_groups(seq_lens: Sequence[int], prefill_group: int, bucket: int = 0) -> List[Tuple[int, int, int]]:
    """How `caption_batch` cuts its clips into prefill passes: [(first clip, clips, stride)], in order, every clip once; neighbours
    share a pass while their strides are equal, at most `prefill_group` of them."""
    out, b, n = [], 0, len(seq_lens)
    while b < n:
        st, g = prompt_stride(seq_lens[b], bucket), 1
        while b + g < n and g < prefill_group and prompt_stride(seq_lens[b + g], bucket) == st:
            g += 1
        out.append((b, g, st))
        b += g
    return out


def check_seq_lens(seq_lens: Sequence[int], stride: int, max_new: int, max_ctx: int, pos0: int = 0) -> List[int]:
    """The host-side half of the variable-length prefill's contract (the kernels only clamp): 1 <= len <= stride, stride a multiple
    of 32, pos0 + len + max_new <= max_ctx (pos0 > 0: the lengths of an `extend_*` pass, which starts at that position)."""
    lens = [int(x) for x in seq_lens]
    if stride < 32 or stride % 32:
        raise ValueError(f"stride {stride} is not a positive multiple of 32")
    for x in lens:
        if not 1 <= x <= stride:
            raise ValueError(f"sequence length {x} outside [1, stride {stride}]")
        if pos0 + x + max_new > max_ctx:
            raise ValueError(f"prompt of {pos0 + x} positions + {max_new} new tokens exceeds max_ctx {max_ctx}")
    return lens


# ---- shared visual prefixes: several prompts about one clip agree on every row up to and including the last visual token
FORK_TOKENS = 64              # a fork lies on a KV page boundary: whole pages are copied, the rest is prefilled (`extend_*`)


def _row_sources(plan: dict) -> np.ndarray:
    """What each row of a spliced prompt is made of: visual row k (in marker order) -> -(k + 1), a text row -> its token id."""
    def host(a):
        return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    src = np.zeros(int(plan["seq_len"]), np.int64)
    vr = host(plan["vis_rows"]).astype(np.int64)
    src[vr] = -(np.arange(len(vr), dtype=np.int64) + 1)
    tr, ti = host(plan["text_rows"]).astype(np.int64), host(plan["text_ids"]).astype(np.int64)
    src[tr[tr >= 0]] = ti[tr >= 0]
    return src


def shared_prefix_rows(plan_a: dict, plan_b: dict) -> int:
    """Leading rows of two splice plans (`splice_rows`) that are identical: the same visual row index in both, or the same text id
    in both.  Says nothing about the visual rows' CONTENTS - the caller's share key does."""
    a = plan_a["row_src"] if "row_src" in plan_a else _row_sources(plan_a)
    b = plan_b["row_src"] if "row_src" in plan_b else _row_sources(plan_b)
    n = min(len(a), len(b))
    diff = np.nonzero(a[:n] != b[:n])[0]
    return int(diff[0]) if len(diff) else n


def fork_point(rows: int) -> int:
    """The position a sibling prompt forks off at: `rows` shared rows rounded down to whole KV pages.  0 = no sharing."""
    return max(int(rows), 0) // FORK_TOKENS * FORK_TOKENS


def _vis_end(plan: dict) -> int:
    """rows up to and including a plan's last visual row"""
    if "vis_end" in plan:
        return plan["vis_end"]
    return int(max(plan["vis_rows"])) + 1 if len(plan["vis_rows"]) else 0


def share_fork(parent: dict, child: dict) -> int:
    """Where `child` may fork off `parent`'s KV sequence (both plans of the SAME visual input), or 0 when it must take the unshared
    path: the plans diverge before the visual rows end, or less than a page is shared.  The child keeps at least one row of its own
    (identical prompts fork a page early: the first token comes from the child's own last row)."""
    if parent["nvis"] != child["nvis"] or parent["used"] != child["used"] or child["nvis"] < 1:
        return 0
    shared = shared_prefix_rows(parent, child)
    if shared < max(_vis_end(parent), _vis_end(child)):
        return 0
    return fork_point(min(shared, int(child["seq_len"]) - 1))


def splice_rows(input_ids: Sequence[int], frames: int, n_kept, strict: bool = False, ntext_cap: Optional[int] = None) -> dict:
    """The row maps of `AuroraCapEngine.splice_plan` as numpy arrays (no device).  ntext_cap: the text arrays are padded to this many
    entries with (id 0, row -1); the splice skips entries whose row is negative."""
    counts = [int(n_kept)] * frames if np.isscalar(n_kept) else [int(c) for c in n_kept]   # per-frame rows (slow-fast: ragged)
    vis_rows, text_ids, text_rows = [], [], []
    row, k = 0, 0
    for tid in input_ids:
        if tid == IMAGE_TOKEN_INDEX:
            if k < frames:
                vis_rows.append(np.arange(row, row + counts[k]))
                row += counts[k]
            elif strict:
                raise IndexError(f"image marker {k} has no frame ({frames} frames)")      # model/utils.py:361
            k += 1
        else:
            text_ids.append(int(tid))
            text_rows.append(row)
            row += 1
    ntext = len(text_ids)
    if ntext_cap is not None:
        if ntext > ntext_cap:
            raise ValueError(f"{ntext} text tokens exceed ntext_cap {ntext_cap}")
        text_ids += [0] * (ntext_cap - ntext)
        text_rows += [-1] * (ntext_cap - ntext)
    vr = np.concatenate(vis_rows) if vis_rows else np.zeros(0, np.int64)
    src = np.zeros(row, np.int64)                      # per row: visual row k -> -(k + 1), text -> its id (`shared_prefix_rows`)
    src[vr] = -(np.arange(len(vr), dtype=np.int64) + 1)
    src[np.asarray(text_rows[:ntext], np.int64)] = np.asarray(text_ids[:ntext], np.int64)
    return dict(row_src=src, vis_end=int(vr.max()) + 1 if len(vr) else 0, seq_len=row, used=len(vis_rows), n_kept=n_kept, nvis=int(sum(counts[:len(vis_rows)])), ntext=ntext, ntext_cap=ntext_cap,
                vis_rows=vr.astype(np.int32), text_ids=np.asarray(text_ids, np.int32), text_rows=np.asarray(text_rows, np.int32))


def front_end_bucket_key(bank: int, front_cus: int, frames: int, height: int, width: int, r: int, seq: int, plan: dict, bucket: int):
    """The key under which `caption_stream` keeps a captured front end.  bucket 0: the exact prompt (its length is a kernel argument
    frozen into the graph).  Otherwise the length is replaced by the stride and the text count by its capacity, both rounded up to
    the bucket: the lengths and the padded text arrays are static device buffers refilled per clip."""
    if bucket:
        return (bank, front_cus, frames, height, width, r, seq, prompt_stride(plan["seq_len"], bucket), plan["used"], plan["nvis"],
                _rup(max(plan["ntext"], 1), bucket), "var")
    return (bank, front_cus, frames, height, width, r, seq, plan["seq_len"], plan["used"], plan["nvis"], plan["ntext"])


# ---- scoring given continuations (`AuroraCapEngine.loglikelihood_batch`): the host-side layout, no device
def loglik_ids(context_ids: Sequence[int], continuation_ids: Sequence[int]) -> List[int]:
    """The prompt a continuation is scored from: context + continuation[:-1] - the last continuation token is only ever a target
    (`aurora_amd.scoring`).  The context may hold image markers (-200); a continuation is plain token ids."""
    cont = [int(t) for t in continuation_ids]
    if any(t < 0 for t in cont):
        raise ValueError("a continuation holds token ids only (no image marker)")
    return [int(t) for t in context_ids] + cont[:-1]


def loglik_entries(ctx_lens: Sequence[int], conts: Sequence[Sequence[int]], stride: int, pos0: int = 0):
    """Entry arrays of one scoring pass (`aur_llm_score_var`): sequence i of the pass holds positions [pos0, ctx_lens[i] + n_i - 1) of
    a context of ctx_lens[i] SPLICED positions followed by conts[i][:-1], `stride` rows apart.  Token j of continuation i is scored
    from position ctx_lens[i] - 1 + j, flat row i * stride + that position - pos0.
    -> (rows int32, targets int32, [(first entry, entries)] per sequence)."""
    rows, targets, spans = [], [], []
    for i, (lc, cont) in enumerate(zip(ctx_lens, conts)):
        n = len(cont)
        first = int(lc) - 1 - pos0
        if n < 1 or first < 0 or first + n > stride:
            raise ValueError(f"sequence {i}: rows [{first}, {first + n}) of a continuation of {n} tokens outside its stride of {stride}")
        spans.append((len(rows), n))
        rows += [i * stride + first + j for j in range(n)]
        targets += [int(t) for t in cont]
    return np.asarray(rows, np.int32), np.asarray(targets, np.int32), spans


def loglik_share_plan(plans: Sequence[dict], ctx_lens: Sequence[int], pixel_keys: Sequence, share: bool = True):
    """Which items of a `loglikelihood_batch` chunk take the shared-prefix route: [(head, [(child, fork), ...])] in item order, every
    item once.  A head runs the whole front end.  A child directly follows its head (or the head's earlier children), is about the
    same pixels (equal `pixel_keys`), and its plan agrees with the head's through the last visual row (`share_fork`); its fork lies
    at or below its first scored position ctx_len - 1, so every scored row belongs to the pass that starts at the fork."""
    out: List[Tuple[int, List[Tuple[int, int]]]] = []
    for i, plan in enumerate(plans):
        if share and out:
            h = out[-1][0]
            if pixel_keys[h] is not None and pixel_keys[h] == pixel_keys[i]:
                fork = min(share_fork(plans[h], plan), fork_point(int(ctx_lens[i]) - 1))
                if fork > 0:
                    out[-1][1].append((i, fork))
                    continue
        out.append((i, []))
    return out


class _PrefixHolders:
    """`caption_stream(share_key=)`'s cache: key -> the KV sequence that holds the leading pages of the first clip of that key, its
    kept visual rows and its splice plan.  Least recently used out.  Lives for one caption_stream call."""

    def __init__(self, seqs: Sequence[int]):
        from collections import OrderedDict
        self.free = list(seqs)
        self.entries = OrderedDict()
        self.plans = {}                                  # (prompt, frames, rows per frame, fork) -> (device splice plan, device length)

    def get(self, key):
        e = self.entries.get(key)
        if e is not None:
            self.entries.move_to_end(key)
        return e

    def put(self, key, **entry) -> Optional[dict]:
        """a holder sequence for `key`: a free one, or the least recently used entry's; None without capacity"""
        if key in self.entries:
            seq = self.entries.pop(key)["seq"]
        elif self.free:
            seq = self.free.pop()
        elif self.entries:
            seq = self.entries.popitem(last=False)[1]["seq"]
        else:
            return None
        self.entries[key] = dict(entry, seq=seq)
        return self.entries[key]


@dataclass(frozen=True)
class _BankState:
    """Host view of one generation bank: the batch and max_new of its last accepted begin_batch."""
    batch: int = 0
    max_new: int = 0


class AuroraCapEngine:
    def __init__(self, cfg: dict, weights: dict, *, max_frames: int = 8, max_batch: int = 1, max_ctx: int = 4096,
                 max_new_tokens: int = 256, page_tokens: int = 64, use_graph: bool = True, num_banks: int = 1,
                 max_image: Optional[int] = None, device: str = "cuda:0", spare_slots: int = 0, prompt_bucket: int = 0,
                 prefix_cache: int = 0):
        # prompt_bucket: 0 = prompts are prefilled at their exact length (equal lengths share a pass, one captured front end per
        # length); 32 / 64 / 128 = at the next multiple of it, lengths in device memory (`prefill_groups`, `front_end_bucket_key`)
        self.prompt_bucket = check_prompt_bucket(prompt_bucket)
        # prefix_cache: how many of the spare KV sequences (the last ones) `caption_stream(share_key=)` keeps as HOLDERS of a keyed
        # clip's leading pages, for later clips of the same key to copy from; they are never a target of a commit's row exchange
        if not 0 <= int(prefix_cache) <= max(int(spare_slots), 0):
            raise ValueError(f"prefix_cache {prefix_cache} outside [0, spare_slots {spare_slots}]")
        self.prefix_cache = int(prefix_cache)
        if not torch.cuda.is_available():
            raise _lib.AuroraHipError("AuroraCapEngine needs a ROCm GPU (torch.cuda.is_available() is False); "
                                      "there is no CPU fallback")
        self.L = _lib.lib()
        self.dev = self.normalize_device(device)
        torch.cuda.set_device(self.dev)
        # All work is enqueued on ONE explicit (non-null) HIP stream: the null stream cannot be captured into
        # a hipGraph.  It becomes this thread's current torch stream, so caller-side tensor housekeeping is
        # ordered with the kernels without cross-stream events.
        self._prev_stream = torch.cuda.current_stream(self.dev)
        self.stream = torch.cuda.Stream(self.dev)
        self.stream.wait_stream(self._prev_stream)
        torch.cuda.set_stream(self.stream)
        self.cfg = cfg
        v, l = cfg.get("vit"), cfg.get("llm")
        c = AurConfig()
        # unused sub-models get harmless valid dims so that aur_create's checks pass
        vv = v or dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=2, intermediate_size=64, patch_size=14,
                       image_size=28, hidden_act="quick_gelu")
        ll = l or dict(hidden_size=128, num_attention_heads=4, num_hidden_layers=1, intermediate_size=128, vocab_size=128,
                       rms_norm_eps=1e-5, rope_theta=1e4)
        c.vit_hidden, c.vit_heads, c.vit_layers = vv["hidden_size"], vv["num_attention_heads"], vv["num_hidden_layers"]
        # vit_image is the CAPACITY (largest input side the workspace admits); the checkpoint's position table belongs to
        # image_size.  max_image > image_size admits larger inputs through the interpolated table (aurora.py:909-951).
        self.max_image = max(int(max_image or 0), vv["image_size"]) // vv["patch_size"] * vv["patch_size"]
        c.vit_mlp, c.vit_patch, c.vit_image = vv["intermediate_size"], vv["patch_size"], self.max_image
        c.vit_native_image = vv["image_size"]
        c.vit_channels = vv.get("num_channels", 3)
        act = vv.get("hidden_act", "quick_gelu")
        if act not in ("quick_gelu", "gelu"):
            raise ValueError(f"unsupported ViT hidden_act {act!r}")
        c.vit_act = _lib.AUR_ACT_GELU if act == "gelu" else _lib.AUR_ACT_QUICK_GELU
        c.vit_ln_eps = vv.get("layer_norm_eps", 1e-5)
        c.llm_hidden, c.llm_heads, c.llm_layers = ll["hidden_size"], ll["num_attention_heads"], ll["num_hidden_layers"]
        c.llm_mlp, c.llm_vocab = ll["intermediate_size"], ll["vocab_size"]
        c.llm_rms_eps, c.rope_theta, c.rope_factor = ll["rms_norm_eps"], ll["rope_theta"], ll.get("rope_factor", 1.0)
        c.max_frames, c.max_batch, c.max_ctx = max_frames, max_batch, max_ctx
        c.max_new_tokens, c.page_tokens, c.use_graph = max_new_tokens, page_tokens, int(use_graph)
        c.num_banks = num_banks
        c.spare_slots = spare_slots
        # projector (configuration_projector.py:9-22): depth / hidden_act / bias come from projector/config.json (cfg["projector"],
        # aurora_amd.checkpoint.projector_config); without one: the AuroraCap defaults, whose depth is read off the weight keys
        pc = dict(cfg.get("projector") or {})
        if "depth" not in pc and "projector" in weights:
            pc["depth"] = sum(1 for k in weights["projector"] if k.endswith(".weight"))
        self.proj_cfg = projector_settings(pc, vv["hidden_size"] if v else None, ll["hidden_size"] if l else None)
        c.proj_depth, c.proj_act = self.proj_cfg["depth"], _lib.ACT_BY_NAME[self.proj_cfg["hidden_act"]]
        self.spare_slots = spare_slots
        self._front_graphs = {}                          # (bank, front-end CUs, shape bucket) -> caption_stream's FrontEndGraph, LRU order
        self.front_graph_cap = 16
        self._banks = [_BankState(), _BankState()]       # the C side's current bank is self._bank
        self._bank = 0
        self._sampling_mode = False                      # ctx option "sampling": flipped by the first sampling request, sticky
        self._samp_stage = None                          # device staging of aur_sampling records, one row per (bank, slot)
        self._rules_mode = False                         # ctx option "logit_rules": flipped by the first request with non-neutral rules, sticky
        self._guid_mode = False                          # ctx option "guidance": flipped by the first guided request, sticky
        self._guid_stage = None                          # device staging of aur_guidance records, one row per (bank, slot)
        self._rules_stage = None                         # device staging of aur_logit_rules records, one row per (bank, slot)
        self._stop_mode = False                          # ctx option "stop_rules": flipped by the first request with a non-neutral stop record, sticky
        self._stop_stage = None                          # device staging of aur_stop_rules records, one row per (bank, slot)
        self._stop_table = None                          # set_stop_vocab: the tokenizer's byte table on the host (validation, finish_reason) ...
        self._stop_table_dev = None                      # ... and on the device (caller-owned memory of aur_stop_vocab)
        self._lp_bufs: Dict[int, torch.Tensor] = {}      # bank -> the caller-owned state of aur_logprob_enable (kept once allocated)
        self._lp_top: Dict[int, int] = {}                # bank -> top_n it records with; absent = off
        self._am_bufs: Dict[int, torch.Tensor] = {}      # bank -> the caller-owned state of aur_attn_map_enable (kept once allocated)
        self._am_on: Dict[int, tuple] = {}               # bank -> (window, layers or None) it records with; absent = off
        self.c = c
        self.v, self.l = v, l
        self.max_new_tokens = max_new_tokens
        self.max_batch = max_batch
        self.ctx = C.c_void_p()
        rc = self.L.aur_create(C.byref(c), C.byref(self.ctx))
        if rc != 0:
            raise _lib.AuroraHipError(f"aur_create failed ({rc}): {self.L.aur_last_error(None).decode()}")
        self._keep: List[torch.Tensor] = []
        self.ws = torch.empty(self.L.aur_workspace_bytes(self.ctx), dtype=torch.uint8, device=self.dev)
        check(self.ctx, self.L.aur_set_workspace(self.ctx, self.ws.data_ptr(), self.ws.numel()), "aur_set_workspace")
        self.kv = None
        if l is not None:
            self.kv = torch.empty(self.L.aur_kv_pool_bytes(self.ctx), dtype=torch.uint8, device=self.dev)
            check(self.ctx, self.L.aur_set_kv_pool(self.ctx, self.kv.data_ptr(), self.kv.numel()), "aur_set_kv_pool")
        if v is not None and "vit" in weights:
            self._load_vit(weights["vit"])
        if l is not None and "llm" in weights:
            self._load_llm(weights["llm"])
            if "projector" in weights:
                self._load_projector(weights["projector"])
        if (v is not None and "vit" in weights) or (l is not None and "llm" in weights):
            check(self.ctx, self.L.aur_finalize(self.ctx, self._stream()), "aur_finalize")
        torch.cuda.synchronize()

    # ------------------------------------------------------------------ housekeeping
    @staticmethod
    def normalize_device(device) -> torch.device:
        """"cuda" (no ordinal, the lmms-eval adaptor's default) -> the process's current GPU: torch.cuda.set_device and the
        allocations below need an indexed device."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.AuroraHipError(f"AuroraCapEngine runs on a ROCm GPU only (device={device!r}); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    def close(self):
        if getattr(self, "ctx", None):
            torch.cuda.synchronize()
            self._front_graphs = {}                                 # the graphs themselves die with the ctx
            self.L.aur_destroy(self.ctx)
            self.ctx = None
            self._masked = {}                                       # CU-masked streams are shared per process (streams.py): never destroyed
            if torch.cuda.current_stream(self.dev) == self.stream:
                torch.cuda.set_stream(self._prev_stream)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        cur = torch.cuda.current_stream(self.dev)
        if cur.cuda_stream != 0:            # any explicit stream the caller made current (e.g. a second pipeline stream)
            return C.c_void_p(cur.cuda_stream)
        self.stream.wait_stream(cur)        # null stream: order ours after it (it cannot be graph-captured)
        return C.c_void_p(self.stream.cuda_stream)

    def _h(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.dev, dtype=torch.float16).contiguous()

    def _f(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.dev, dtype=torch.float32).contiguous()

    def _set(self, name: str, t: torch.Tensor):
        self._keep.append(t)
        check(self.ctx, self.L.aur_set_tensor(self.ctx, name.encode(), t.data_ptr(), t.numel() * t.element_size()), name)

    def pack(self, w: torch.Tensor, npad: int, kpad: int, row_map: Optional[np.ndarray] = None) -> torch.Tensor:
        """row-major [N, K] -> MFMA fragment tiles (aur_pack_linear)."""
        w = self._h(w)
        n, k = w.shape
        out = torch.empty(npad * kpad, dtype=torch.float16, device=self.dev)
        rm = None
        if row_map is not None:
            assert row_map.shape[0] == npad
            rm = torch.from_numpy(row_map.astype(np.int32)).to(self.dev)
        check(self.ctx, self.L.aur_pack_linear(self.ctx, w.data_ptr(), n, k, k, rm.data_ptr() if rm is not None else None,
                                               npad, kpad, out.data_ptr(), self._stream()), "aur_pack_linear")
        torch.cuda.current_stream().synchronize()
        return out

    def _bias(self, b: Optional[torch.Tensor], npad: int, row_map: Optional[np.ndarray] = None) -> torch.Tensor:
        out = torch.zeros(npad, dtype=torch.float32, device=self.dev)
        if b is None:
            return out
        b = self._f(b)
        if row_map is None:
            out[: b.numel()] = b
        else:
            rm = torch.from_numpy(row_map.astype(np.int64)).to(self.dev)
            ok = rm >= 0
            out[ok] = b[rm[ok]]
        return out

    # ------------------------------------------------------------------ weight loading
    def _load_vit(self, w: dict):
        v = self.v
        D, H, mlp = v["hidden_size"], v["num_attention_heads"], v["intermediate_size"]
        hd = D // H
        hdp = _rup(hd, 32)
        qcols = _rup(H * hdp, 64)
        npad = _rup(2 * qcols + D, 256)
        dpad, mpad = _rup(D, 256), _rup(mlp, 256)
        P, Cn = v["patch_size"], v.get("num_channels", 3)
        kpad = _rup(Cn * P * P, 64)
        rm = self.vit_qkv_row_map(D, H, npad)
        self._set("vit.patch.w", self.pack(w["patch_embedding.weight"].reshape(D, -1), dpad, kpad))
        self._set("vit.cls", self._h(w["class_embedding"].reshape(-1)))
        self._pos_cache: Dict[tuple, torch.Tensor] = {}                  # interpolated_pos(): one table per input size
        self._set("vit.pos", self._h(w["position_embedding.weight"]))
        self._set("vit.preln.w", self._f(w["pre_layrnorm.weight"]))
        self._set("vit.preln.b", self._f(w["pre_layrnorm.bias"]))
        nl = v["num_hidden_layers"] - 1          # hidden_states[-2]: the last layer is never needed
        for i in range(nl):
            lw = w["layers"][i]
            p = f"vit.{i}."
            for a in ("ln1", "ln2"):
                full = "layer_norm1" if a == "ln1" else "layer_norm2"
                self._set(p + a + ".w", self._f(lw[full + ".weight"]))
                self._set(p + a + ".b", self._f(lw[full + ".bias"]))
            wqkv = torch.cat([lw["q_proj.weight"], lw["k_proj.weight"], lw["v_proj.weight"]], 0)
            bqkv = torch.cat([lw["q_proj.bias"], lw["k_proj.bias"], lw["v_proj.bias"]], 0)
            self._set(p + "qkv.w", self.pack(wqkv, npad, D, rm))
            self._set(p + "qkv.b", self._bias(bqkv, npad, rm))
            self._set(p + "out.w", self.pack(lw["out_proj.weight"], dpad, D))
            self._set(p + "out.b", self._bias(lw["out_proj.bias"], dpad))
            self._set(p + "fc1.w", self.pack(lw["fc1.weight"], mpad, D))
            self._set(p + "fc1.b", self._bias(lw["fc1.bias"], mpad))
            self._set(p + "fc2.w", self.pack(lw["fc2.weight"], dpad, mlp))
            self._set(p + "fc2.b", self._bias(lw["fc2.bias"], dpad))

    @staticmethod
    def vit_qkv_row_map(D: int, heads: int, npad: int) -> np.ndarray:
        """fused QKV row map of the vision tower: Q and K heads padded hd -> hd_pad (zero rows), V natural"""
        hd = D // heads
        hdp = _rup(hd, 32)
        qcols = _rup(heads * hdp, 64)
        rm = np.full(npad, -1, np.int32)
        for h in range(heads):
            rm[h * hdp: h * hdp + hd] = np.arange(h * hd, (h + 1) * hd)
            rm[qcols + h * hdp: qcols + h * hdp + hd] = D + np.arange(h * hd, (h + 1) * hd)
        rm[2 * qcols: 2 * qcols + D] = 2 * D + np.arange(D)
        return rm

    @staticmethod
    def llama_qkv_row_map(d: int, heads: int, npad: int) -> np.ndarray:
        """Q/K rows permuted per head so that fragment tile 2p holds d in [16p, 16p+16) and tile 2p+1 its RoPE
        partner d + hd/2: the rotation (HF rotate_half) happens in-lane in the GEMM epilogue."""
        hd = d // heads
        rm = np.full(npad, -1, np.int32)
        per_head = np.empty(hd, np.int64)
        for p in range(hd // 32):
            per_head[32 * p: 32 * p + 16] = 16 * p + np.arange(16)
            per_head[32 * p + 16: 32 * p + 32] = hd // 2 + 16 * p + np.arange(16)
        for h in range(heads):
            rm[h * hd: (h + 1) * hd] = h * hd + per_head
            rm[d + h * hd: d + (h + 1) * hd] = d + h * hd + per_head
        rm[2 * d: 3 * d] = 2 * d + np.arange(d)
        return rm

    @staticmethod
    def gateup_row_map(mlp: int, npad: int) -> np.ndarray:
        """fused gate/up row map: packed row 2j = gate row j, 2j + 1 = up row j (row mlp + j of [gate; up]), so that one lane of the
        SiLU*up epilogue holds both halves of h[j]"""
        rm = np.full(npad, -1, np.int32)
        rm[0: 2 * mlp: 2] = np.arange(mlp)
        rm[1: 2 * mlp: 2] = mlp + np.arange(mlp)
        return rm

    def _load_llm(self, w: dict):
        l = self.l
        d, H, mlp, V = l["hidden_size"], l["num_attention_heads"], l["intermediate_size"], l["vocab_size"]
        qkv_npad, gu_npad, dpad, vpad = _rup(3 * d, 256), _rup(2 * mlp, 256), _rup(d, 256), _rup(V, 256)
        rm_qkv = self.llama_qkv_row_map(d, H, qkv_npad)
        rm_gu = self.gateup_row_map(mlp, gu_npad)
        # RMSNorm weights are FOLDED into the projection that consumes the normalised activations:
        #   W (w_norm * x_hat) = (W diag(w_norm)) x_hat.  The kernels then only need the per-row 1/rms
        #   (prefill: weight-less norm kernel; decode: sum(x^2) carried by the residual-producing epilogues).
        def fold(wmat, wnorm):
            return (wmat.detach().to(self.dev, torch.float32) * wnorm.detach().to(self.dev, torch.float32)[None, :]).to(torch.float16)

        self._set("llm.embed", self._h(w["embed_tokens.weight"]))
        self._set("llm.lm_head.w", self.pack(fold(w["lm_head.weight"], w["norm.weight"]), vpad, d))
        for i, lw in enumerate(w["layers"]):
            p = f"llm.{i}."
            wqkv = torch.cat([lw["q_proj.weight"], lw["k_proj.weight"], lw["v_proj.weight"]], 0)
            self._set(p + "qkv.w", self.pack(fold(wqkv, lw["input_layernorm.weight"]), qkv_npad, d, rm_qkv))
            self._set(p + "o.w", self.pack(lw["o_proj.weight"], dpad, d))
            wgu = torch.cat([lw["gate_proj.weight"], lw["up_proj.weight"]], 0)
            self._set(p + "gateup.w", self.pack(fold(wgu, lw["post_attention_layernorm.weight"]), gu_npad, d, rm_gu))
            self._set(p + "down.w", self.pack(lw["down_proj.weight"], dpad, mlp))

    def _load_projector(self, w: dict):
        """modeling_projector.py:20-33: `model.0`, then (`ACT2FN[hidden_act]`, `model.2k`) for k = 1 .. depth - 1.  A bias-free projector
        (`bias=False`) loads zeros.  Keys, shapes and count are checked against the config: nothing loads silently wrong."""
        d, dv, pc = self.l["hidden_size"], self.v["hidden_size"], self.proj_cfg
        dpad = _rup(d, 256)
        want = {f"model.{2 * i}.weight" for i in range(pc["depth"])}
        have = {k for k in w if k.endswith(".weight")}
        if want != have:
            raise ValueError(f"projector weights {sorted(have)} do not match depth {pc['depth']} (expected {sorted(want)})")
        for i in range(pc["depth"]):
            wt, k_in = w[f"model.{2 * i}.weight"], (dv if i == 0 else d)
            if tuple(wt.shape) != (d, k_in):
                raise ValueError(f"projector model.{2 * i}.weight has shape {tuple(wt.shape)}, the configs say {(d, k_in)}")
            b = w.get(f"model.{2 * i}.bias")
            if (b is not None) != pc["bias"]:
                raise ValueError(f"projector model.{2 * i}.bias {'present' if b is not None else 'missing'} but config.bias is {pc['bias']}")
            self._set(f"proj.{i}.w", self.pack(wt, dpad, k_in))
            self._set(f"proj.{i}.b", self._bias(b if b is not None else torch.zeros(d), dpad))

    # ------------------------------------------------------------------ hot path
    def tome_r(self, token_kept_ratio: float, height: Optional[int] = None, width: Optional[int] = None) -> int:
        v = self.v
        return tome_r(height or v["image_size"], width or v["image_size"], v["patch_size"], token_kept_ratio,
                      v["num_hidden_layers"])

    def vit_encode(self, pixels: torch.Tensor, r: int, out: Optional[torch.Tensor] = None, merge_map: bool = False):
        """pixels [F, C, H, W] -> hidden_states[-2][:, 1:]  as fp16 [F, n_kept, D] (into `out` when given: a captured front
        end must not allocate).  merge_map=True: (tokens, map int32 [F, gh, gw], sizes fp32 [F, n_kept]) - map[f, y, x] is the row of
        tokens[f] that patch (y, x) was merged into, sizes[f, k] the number of patches in row k (`aurora_amd.merge_map`); the
        tokens are bitwise those of the plain call; `out` is then the three tensors, (tokens, map, sizes)."""
        v = self.v
        if pixels.dim() != 4 or pixels.shape[1] != v.get("num_channels", 3):
            raise ValueError(f"pixel_values must be [frames, {v.get('num_channels', 3)}, H, W], got {tuple(pixels.shape)}")
        px = self._h(pixels)
        F, H, W = px.shape[0], px.shape[-2], px.shape[-1]
        t0 = (H // v["patch_size"]) * (W // v["patch_size"]) + 1
        if t0 < 2 or t0 > (self.max_image // v["patch_size"]) ** 2 + 1:
            raise ValueError(f"a {H}x{W} input has {t0} tokens per frame; this engine holds up to "
                             f"{(self.max_image // v['patch_size']) ** 2 + 1} (max_image {self.max_image})")
        n_kept = tokens_at_layer(t0, r, v["num_hidden_layers"] - 1) - 1
        mp = sz = None
        if merge_map and out is not None:                   # a captured call brings all three: (tokens, map, sizes)
            out, mp, sz = out
            grid = (F, H // v["patch_size"], W // v["patch_size"])
            assert mp.shape == grid and mp.dtype == torch.int32 and mp.is_contiguous() and mp.is_cuda
            assert sz.shape == (F, n_kept) and sz.dtype == torch.float32 and sz.is_contiguous() and sz.is_cuda
        if out is None:
            out = torch.empty(F, n_kept, v["hidden_size"], dtype=torch.float16, device=self.dev)
        else:
            assert out.shape == (F, n_kept, v["hidden_size"]) and out.dtype == torch.float16 and out.is_contiguous() and out.is_cuda
        nk = C.c_int32(0)
        pos = self.interpolated_pos(H, W)
        if merge_map:
            if mp is None:
                mp = torch.empty(F, H // v["patch_size"], W // v["patch_size"], dtype=torch.int32, device=self.dev)
                sz = torch.empty(F, n_kept, dtype=torch.float32, device=self.dev)
            check(self.ctx, self.L.aur_vit_encode_map(self.ctx, px.data_ptr(), F, H, W, pos.data_ptr() if pos is not None else None, r,
                                                      out.data_ptr(), mp.data_ptr(), sz.data_ptr(), C.byref(nk), self._stream()),
                  "aur_vit_encode_map")
            assert nk.value == n_kept
            return out, mp, sz
        check(self.ctx, self.L.aur_vit_encode_hw(self.ctx, px.data_ptr(), F, H, W, pos.data_ptr() if pos is not None else None, r,
                                                 out.data_ptr(), C.byref(nk), self._stream()), "aur_vit_encode")
        assert nk.value == n_kept
        return out

    def interpolated_pos(self, height: int, width: int) -> Optional[torch.Tensor]:
        """Position table for a non-native input size (aurora.py:909-951): the n x n patch rows of the checkpoint's table
        resampled bicubically to (height // patch, width // patch) with the reference's scale factors (g + 0.1) / n; None
        for the native grid.  One launch per input size (`pos_interp_kernel`, vit.hip), cached."""
        v = self.v
        gh, gw = height // v["patch_size"], width // v["patch_size"]
        n = v["image_size"] // v["patch_size"]
        if gh == n and gw == n:
            return None
        key = (gh, gw)
        if key not in self._pos_cache:
            tab = torch.empty(1 + gh * gw, v["hidden_size"], dtype=torch.float16, device=self.dev)
            check(self.ctx, self.L.aur_vit_pos_interp(self.ctx, height, width, tab.data_ptr(), self._stream()), "aur_vit_pos_interp")
            self._pos_cache[key] = tab
        return self._pos_cache[key]

    def splice_plan(self, input_ids: Sequence[int], frames: int, n_kept, strict: bool = False, ntext_cap: Optional[int] = None):
        """Destination-row maps of the prefix splice for one prompt (model/utils.py:198-240 semantics: marker k takes
        frame k; markers beyond the number of frames are dropped), uploaded once.  Re-usable across calls: building it
        involves blocking host->device copies, which must stay out of a multi-stream pipeline's steady state.
        ntext_cap: pad the text arrays to that many entries (row -1 = unused) for the strided splice (`project_splice(stride=)`)."""
        p = splice_rows(input_ids, frames, n_kept, strict, ntext_cap)
        p["len_dev"] = torch.tensor([p["seq_len"]], dtype=torch.int32, device=self.dev)      # what a variable-length prefill reads
        for k in ("vis_rows", "text_ids", "text_rows"):
            p[k] = torch.from_numpy(p[k]).to(self.dev)
        return p

    def project_splice(self, vis: torch.Tensor, input_ids: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None,
                       plan: Optional[dict] = None, stride: Optional[int] = None):
        """vis [frames, n_kept, Dv] + ids (with -200 markers) -> (embeds [L_pad, d] fp16, seq_len).
        stride: the strided form for a variable-length prefill - embeds holds `stride` rows, every entry of the plan's text arrays
        is passed (entries with row -1 are skipped on the device, `splice_plan(ntext_cap=)`), no padding row is cleared here."""
        d = self.l["hidden_size"]
        if vis.dim() == 2:                    # flat rows in marker order (frames with different token counts: slow-fast)
            assert plan is not None and plan["nvis"] <= vis.shape[0]
            seq_len = plan["seq_len"]
            vflat = self._h(vis[:plan["nvis"]])
        else:
            if plan is None:
                plan = self.splice_plan(input_ids, vis.shape[0], vis.shape[1])
            assert plan["n_kept"] == vis.shape[1] and plan["used"] <= vis.shape[0]
            seq_len, used = plan["seq_len"], plan["used"]
            vflat = self._h(vis[:used]).reshape(used * plan["n_kept"], vis.shape[-1])      # used may be 0: a text-only splice
        rows = _rup(seq_len, 32) if stride is None else stride
        embeds = out if out is not None else torch.empty(rows, d, dtype=torch.float16, device=self.dev)
        assert embeds.shape[0] >= rows and embeds.is_contiguous()
        if stride is not None:
            if seq_len > stride:
                raise ValueError(f"prompt of {seq_len} positions in a stride of {stride}")
            check(self.ctx, self.L.aur_project_splice_var(self.ctx, vflat.data_ptr(), vflat.shape[0], plan["vis_rows"].data_ptr(),
                                                          plan["text_ids"].data_ptr(), plan["text_rows"].data_ptr(), plan["text_rows"].numel(),
                                                          stride, embeds.data_ptr(), self._stream()), "aur_project_splice_var")
            self._tmp = getattr(self, "_tmp", [])[-64:] + [(vflat, plan)]
            return embeds, seq_len
        check(self.ctx, self.L.aur_project_splice(self.ctx, vflat.data_ptr(), vflat.shape[0], plan["vis_rows"].data_ptr(),
                                                  plan["text_ids"].data_ptr(), plan["text_rows"].data_ptr(), plan["ntext"], seq_len,
                                                  embeds.data_ptr(), self._stream()), "aur_project_splice")
        self._tmp = getattr(self, "_tmp", [])[-64:] + [(vflat, plan)]      # keep alive until consumed
        return embeds, seq_len

    def select_bank(self, bank: int):
        """Switch the generation bank (double-buffered KV slots / state) that the following calls act on."""
        check(self.ctx, self.L.aur_select_bank(self.ctx, bank), "aur_select_bank")
        self._bank = bank

    @property
    def _batch(self) -> int:
        return self._banks[self._bank].batch

    @property
    def _max_new(self) -> int:
        return self._banks[self._bank].max_new

    def begin_batch(self, batch: int, max_new_tokens: int, eos_id: Optional[int]):
        check(self.ctx, self.L.aur_begin_batch(self.ctx, batch, max_new_tokens, -1 if eos_id is None else int(eos_id),
                                               self._stream()), "aur_begin_batch")
        self._banks[self._bank] = _BankState(batch, max_new_tokens)

    def prefill(self, slot: int, embeds: torch.Tensor, seq_len: int):
        check(self.ctx, self.L.aur_llm_prefill(self.ctx, slot, embeds.data_ptr(), seq_len, self._stream()), "aur_llm_prefill")

    def _lens_arg(self, seq_lens, nseq: int, stride: int, pos0: int = 0) -> torch.Tensor:
        """seq_lens of a variable-length prefill as the int32 device tensor the kernels read: a list is checked here (the only place
        the lengths are known on the host) and uploaded; a device tensor is the caller's promise and is passed through."""
        if torch.is_tensor(seq_lens):
            if seq_lens.dtype != torch.int32 or not seq_lens.is_cuda or not seq_lens.is_contiguous() or seq_lens.numel() < nseq:
                raise ValueError(f"seq_lens must be a contiguous int32 device tensor of at least {nseq} entries")
            if stride < 32 or stride % 32:
                raise ValueError(f"stride {stride} is not a positive multiple of 32")
            return seq_lens
        lens = check_seq_lens(seq_lens, stride, self._max_new, self.c.max_ctx, pos0)
        if len(lens) != nseq:
            raise ValueError(f"{len(lens)} lengths for {nseq} sequences")
        t = torch.tensor(lens, dtype=torch.int32, device=self.dev)
        self._tmp = getattr(self, "_tmp", [])[-64:] + [t]         # keep alive until consumed
        return t

    def _pass(self, kind: str, ids: Sequence[int], embeds: torch.Tensor, t: int, lens, pos0: Optional[int] = None):
        """One prefill pass through the entry point that (kind, has lengths, has pos0) selects.  kind: "batch" / "stage" / "commit"; ids:
        the leading (slot0 or seq0, nseq[, seq0]) arguments; t: the sequence length or, with lengths, the stride; pos0: the extend forms."""
        name = f"aur_llm_{'prefill' if pos0 is None else 'extend'}_{kind}" + ("" if lens is None else "_var")
        args = [*ids, embeds.data_ptr(), *([] if pos0 is None else [pos0]), t]
        if lens is not None:
            args.append(self._lens_arg(lens, ids[1], t, pos0 or 0).data_ptr())
        check(self.ctx, getattr(self.L, name)(self.ctx, *args, self._stream()), name)

    def prefill_batch(self, slot0: int, nseq: int, embeds: torch.Tensor, seq_len: int, seq_lens=None):
        """embeds [nseq * round_up(seq_len, 32), d]: equal-length sequences prefetched in ONE pass (large-M GEMMs).
        seq_lens (a list, or an int32 device tensor): sequences of DIFFERENT lengths, `seq_len` rows apart (a multiple of 32);
        every sequence gets bitwise what it gets alone."""
        self._pass("batch", (slot0, nseq), embeds, seq_len, seq_lens)

    def prefill_stage(self, seq0: int, nseq: int, embeds: torch.Tensor, seq_len: int, seq_lens=None):
        """The layer stack of `prefill_batch` into KV sequences [seq0, seq0 + nseq) (normally the spare ones,
        `max_batch ..`): touches no decode state, so it may run on another stream while `decode` runs."""
        self._pass("stage", (seq0, nseq), embeds, seq_len, seq_lens)

    def prefill_commit(self, slot0: int, nseq: int, seq0: int, embeds: torch.Tensor, seq_len: int, seq_lens=None):
        """On the decode stream, after `prefill_stage` has completed: slots [slot0 ..) take over the pages of sequences
        [seq0 ..) (which get the slots' old pages), are reset, and receive their first tokens."""
        self._pass("commit", (slot0, nseq, seq0), embeds, seq_len, seq_lens)

    # ------------------------------------------------------------------ shared prefixes
    def kv_copy_prefix(self, src_seq: int, dst_seq0: int, ndst: int, tokens: int):
        """K / V of positions [0, tokens) of KV sequence `src_seq` -> sequences [dst_seq0, dst_seq0 + ndst) of the current bank, every
        layer, in one launch that reads the source once (enqueue-only; `tokens` a multiple of the 64-token page)."""
        check(self.ctx, self.L.aur_kv_copy_prefix(self.ctx, src_seq, dst_seq0, ndst, tokens, self._stream()), "aur_kv_copy_prefix")

    def extend_batch(self, slot0: int, nseq: int, embeds: torch.Tensor, pos0: int, stride: int, new_lens):
        """`prefill_batch(seq_lens=)` for slots that already hold positions [0, pos0) (`kv_copy_prefix`, or an earlier prefill): embeds
        [nseq * stride, d], rows [i * stride, i * stride + new_lens[i]) = positions [pos0, pos0 + new_lens[i]).  Bitwise what
        `prefill(slot, full_embeds, pos0 + new_lens[i])` gives.  new_lens: a list (checked here) or an int32 device tensor."""
        self._pass("batch", (slot0, nseq), embeds, stride, new_lens, pos0)

    def extend_stage(self, seq0: int, nseq: int, embeds: torch.Tensor, pos0: int, stride: int, new_lens):
        """The layer stack of `extend_batch` into KV sequences [seq0, seq0 + nseq): touches no decode state (see `prefill_stage`)."""
        self._pass("stage", (seq0, nseq), embeds, stride, new_lens, pos0)

    def extend_commit(self, slot0: int, nseq: int, seq0: int, embeds: torch.Tensor, pos0: int, stride: int, new_lens):
        """`prefill_commit` for sequences staged by `extend_stage` (same pos0, stride and lengths): decode position pos0 + new_lens[i]."""
        self._pass("commit", (slot0, nseq, seq0), embeds, stride, new_lens, pos0)

    def _extend_rows(self, vis: torch.Tensor, plan: dict, fork: int, out: torch.Tensor):
        """Rows [fork, seq_len) of a sibling prompt's spliced embeddings -> out[: seq_len - fork] (its own plan over the kept visual
        rows: the projector runs, the ViT does not)."""
        emb, L = self.project_splice(vis, plan=plan)
        out[:L - fork].copy_(emb[fork:L])

    def decode(self, steps: int):
        check(self.ctx, self.L.aur_llm_decode(self.ctx, steps, self._stream()), "aur_llm_decode")

    def outputs(self, logprobs: Optional[int] = None, count: Optional[int] = None):
        """The generated ids of every slot; with logprobs=n (a bank that records them, `_logprobs_on`) a dict per slot instead:
        ids, token_logprobs float32 [len], top_ids int32 [len, n], top_logprobs float32 [len, n].  count: slots [0, count) only
        (a guided call's leaders)."""
        ids = np.zeros((self._batch, self._max_new), np.int32)
        lens = np.zeros(self._batch, np.int32)
        check(self.ctx, self.L.aur_get_outputs(self.ctx, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                               lens.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()), "aur_get_outputs")
        nb = self._batch if count is None else min(int(count), self._batch)
        out = [ids[b, : lens[b]].tolist() for b in range(nb)]
        if logprobs is None:
            return out
        n = check_logprobs(logprobs)
        rec, lp, tid, tlp = self.token_logprob_state()
        if (rec[:nb] != lens[:nb]).any():
            raise RuntimeError(f"log-probability records {rec.tolist()} for generated lengths {lens.tolist()}: enabled in mid-generation?")
        return [dict(ids=out[b], token_logprobs=lp[b, :lens[b]].copy(), top_ids=tid[b, :lens[b], :n].copy(),
                     top_logprobs=tlp[b, :lens[b], :n].copy()) for b in range(nb)]

    def unfinished(self) -> int:
        n = C.c_int32(0)
        check(self.ctx, self.L.aur_unfinished(self.ctx, C.byref(n), self._stream()), "aur_unfinished")
        return n.value

    def logits(self) -> torch.Tensor:
        """fp32 [batch, vocab] logits of the most recent prefill / decode step (copy)."""
        out = torch.empty(self._batch, self.l["vocab_size"], dtype=torch.float32, device=self.dev)
        check(self.ctx, self.L.aur_copy_logits(self.ctx, out.data_ptr(), self._stream()), "aur_copy_logits")
        torch.cuda.synchronize()
        return out

    # ------------------------------------------------------------------ scoring given continuations
    def score_rows(self, logits: torch.Tensor, targets):
        """The scoring kernel alone (aur_score_rows): logits fp32 [rows, vocab] on the device, one target per row (a list, or an int32
        device tensor) -> (log-probabilities float32, first argmax int32) as numpy.  A target outside [0, vocab): (0, -1)."""
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) == logits.shape[1]
        rows, vocab = logits.shape
        tg = targets if torch.is_tensor(targets) else torch.tensor([int(t) for t in targets], dtype=torch.int32, device=self.dev)
        assert tg.dtype == torch.int32 and tg.is_cuda and tg.numel() >= rows
        lp = torch.empty(rows, dtype=torch.float32, device=self.dev)
        am = torch.empty(rows, dtype=torch.int32, device=self.dev)
        check(self.ctx, self.L.aur_score_rows(self.ctx, logits.data_ptr(), rows, vocab, tg.data_ptr(), lp.data_ptr(), am.data_ptr(), self._stream()),
              "aur_score_rows")
        torch.cuda.synchronize()
        return lp.cpu().numpy(), am.cpu().numpy()

    def _i32_arg(self, a, n: int, what: str) -> torch.Tensor:
        if torch.is_tensor(a):
            if a.dtype != torch.int32 or not a.is_cuda or not a.is_contiguous() or a.numel() < n:
                raise ValueError(f"{what} must be a contiguous int32 device tensor of at least {n} entries")
            return a
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)
        if t.numel() != n:
            raise ValueError(f"{t.numel()} {what} for {n}")
        self._tmp = getattr(self, "_tmp", [])[-64:] + [t]         # keep alive until consumed
        return t

    def score_stage(self, seq0: int, nseq: int, embeds: torch.Tensor, pos0: int, stride: int, lens, rows, targets, *, nscore: Optional[int] = None,
                    logprob_out: Optional[torch.Tensor] = None, argmax_out: Optional[torch.Tensor] = None,
                    logits_out: Optional[torch.Tensor] = None, want_logits: bool = False):
        """aur_llm_score_var: the layer stack of `prefill_stage(seq_lens=)` (pos0 == 0) or `extend_stage` (pos0 > 0) into KV sequences
        [seq0, seq0 + nseq) with the last layer unpruned, then entry j - flat row rows[j] = i * stride + r of embeds, the hidden state
        at position pos0 + r of sequence i - scored against targets[j]; a row of -1 is an unused entry.  lens / rows / targets: lists
        (checked and uploaded here) or int32 device tensors (the caller's promise; `nscore` entries, default all of `rows`).
        Enqueue-only: -> (logprob float32 [nscore], argmax int32 [nscore], logits fp32 [nscore, vocab] or None) on the device."""
        if torch.is_tensor(lens):
            lens_t = self._i32_arg(lens, nseq, "lens")
        else:
            ll = [int(x) for x in lens]
            for x in ll:
                if not 1 <= x <= stride or pos0 + x > self.c.max_ctx:
                    raise ValueError(f"sequence of {x} rows at position {pos0}: outside [1, stride {stride}] or beyond max_ctx {self.c.max_ctx}")
            lens_t = self._i32_arg(ll, nseq, "lens")
        n = int(nscore) if nscore is not None else (rows.numel() if torch.is_tensor(rows) else len(rows))
        rows_t, tg_t = self._i32_arg(rows, n, "score rows"), self._i32_arg(targets, n, "score targets")
        vocab = self.l["vocab_size"]
        lp = logprob_out if logprob_out is not None else torch.empty(n, dtype=torch.float32, device=self.dev)
        am = argmax_out if argmax_out is not None else torch.empty(n, dtype=torch.int32, device=self.dev)
        lg = logits_out if logits_out is not None else (torch.empty(n, vocab, dtype=torch.float32, device=self.dev) if want_logits else None)
        assert lp.dtype == torch.float32 and am.dtype == torch.int32 and lp.numel() >= n and am.numel() >= n
        assert lg is None or (lg.dtype == torch.float32 and lg.is_contiguous() and lg.numel() >= n * vocab)
        if getattr(self, "_score_scratch", None) is None:
            self._score_scratch = torch.empty(self.L.aur_score_scratch_bytes(self.ctx), dtype=torch.uint8, device=self.dev)
        sc = self._score_scratch
        check(self.ctx, self.L.aur_llm_score_var(self.ctx, seq0, nseq, embeds.data_ptr(), pos0, stride, lens_t.data_ptr(), rows_t.data_ptr(),
                                                 tg_t.data_ptr(), n, sc.data_ptr(), sc.numel(), lp.data_ptr(), am.data_ptr(),
                                                 lg.data_ptr() if lg is not None else None, self._stream()), "aur_llm_score_var")
        return lp, am, lg

    def loglikelihood_batch(self, items, token_kept_ratio: float, share: bool = True, prefill_group: int = 8) -> List[dict]:
        """Log-likelihood of given continuations: items = [(pixel_values [f, C, H, W], context_ids with -200 markers, continuation_ids)]
        -> per item dict(logprob = the sum of the tokens' log-probabilities (float64, token order), greedy = every continuation token
        is the first argmax of its row, token_logprobs = [float], count = tokens) - `aurora_amd.scoring` is the definition.
        Each sequence is laid out as context + continuation[:-1] and runs through ONE prefill pass whose rows ctx_len - 1 .. are
        scored (`score_stage`); neighbours whose lengths round up to the same stride share a pass (`prefill_groups`).  An empty
        continuation is (0.0, True) with no GPU work.  Calls `begin_batch` itself, like `caption_batch`: not meant to run beside a
        live `caption_stream`.  ValueError when a sequence does not fit max_ctx.
        share=True: neighbouring items about the same pixels tensor whose plans agree through the last visual row (several candidate
        answers to one question about one clip) take the shared-prefix route - the first runs the whole front end, the others copy
        the common KV pages from it (`kv_copy_prefix`) and are scored in one pass that starts at the fork (`loglik_share_plan`).
        Bitwise the result of share=False."""
        from . import scoring
        results: List[Optional[dict]] = [None] * len(items)
        live = []
        for i, (px, ctx_ids, cont) in enumerate(items):
            cont = [int(t) for t in cont]
            if not cont:
                results[i] = dict(logprob=0.0, greedy=True, token_logprobs=[], count=0)
            else:
                live.append((i, px, loglik_ids(ctx_ids, cont), cont))
        d = self.l["hidden_size"]
        bucket = self.prompt_bucket or 32                          # a scoring pass is always the strided form
        for c0 in range(0, len(live), self.max_batch):
            chunk = live[c0:c0 + self.max_batch]
            rs, plans, ctx_lens = [], [], []
            for _, px, ids, cont in chunk:
                r = self.tome_r(token_kept_ratio, px.shape[-2], px.shape[-1])
                t0 = (px.shape[-2] // self.v["patch_size"]) * (px.shape[-1] // self.v["patch_size"]) + 1     # as vit_encode counts them
                plan = self.splice_plan(ids, px.shape[0], tokens_at_layer(t0, r, self.v["num_hidden_layers"] - 1) - 1)
                if plan["seq_len"] > self.c.max_ctx:
                    raise ValueError(f"context + continuation of {plan['seq_len']} positions exceeds max_ctx {self.c.max_ctx}")
                rs.append(r)
                plans.append(plan)
                ctx_lens.append(plan["seq_len"] - (len(cont) - 1))
            conts = [c[3] for c in chunk]
            keys = [(c[1].data_ptr(), tuple(c[1].shape)) for c in chunk]
            groups = loglik_share_plan(plans, ctx_lens, keys, share)
            heads = [h for h, _ in groups]
            seq_of = {h: k for k, h in enumerate(heads)}           # KV sequences: the heads first, then the children, both in item order
            for _, kids in groups:
                for c, _ in kids:
                    seq_of[c] = len(seq_of)
            keep_vis = {h for h, kids in groups if kids}
            vis_of, pending = {}, []
            self.begin_batch(len(chunk), 1, None)
            for b, g, stride in prefill_groups([plans[h]["seq_len"] for h in heads], prefill_group, bucket):
                members = heads[b:b + g]
                buf = torch.empty(g * stride, d, dtype=torch.float16, device=self.dev)
                for k, h in enumerate(members):
                    vis = self.vit_encode(chunk[h][1], rs[h])
                    if h in keep_vis:
                        vis_of[h] = vis
                    self.project_splice(vis, out=buf[k * stride:(k + 1) * stride], plan=plans[h])
                rows, tg, spans = loglik_entries([ctx_lens[h] for h in members], [conts[h] for h in members], stride)
                lp, am, _ = self.score_stage(seq_of[members[0]], g, buf, 0, stride, [plans[h]["seq_len"] for h in members], rows, tg)
                pending.append((members, spans, lp, am, buf))
            for h, kids in groups:
                k0 = 0
                while k0 < len(kids):                              # neighbouring children of one fork: one copy, one pass
                    fork, g = kids[k0][1], 1
                    while k0 + g < len(kids) and kids[k0 + g][1] == fork and g < prefill_group:
                        g += 1
                    members = [c for c, _ in kids[k0:k0 + g]]
                    new = [plans[c]["seq_len"] - fork for c in members]
                    stride = _rup(max(new), 32)
                    buf = torch.empty(g * stride, d, dtype=torch.float16, device=self.dev)
                    for k, c in enumerate(members):
                        self._extend_rows(vis_of[h], plans[c], fork, buf[k * stride:(k + 1) * stride])
                    self.kv_copy_prefix(seq_of[h], seq_of[members[0]], g, fork)
                    rows, tg, spans = loglik_entries([ctx_lens[c] for c in members], [conts[c] for c in members], stride, fork)
                    lp, am, _ = self.score_stage(seq_of[members[0]], g, buf, fork, stride, new, rows, tg)
                    pending.append((members, spans, lp, am, buf))
                    k0 += g
            torch.cuda.synchronize()
            for members, spans, lp, am, _ in pending:
                lp, am = lp.cpu().numpy(), am.cpu().numpy()
                for m, (e0, n) in zip(members, spans):
                    greedy = bool((am[e0:e0 + n] == np.asarray(conts[m], np.int32)).all())
                    total, greedy, lps = scoring.combine(lp[e0:e0 + n].tolist(), greedy)
                    results[chunk[m][0]] = dict(logprob=total, greedy=greedy, token_logprobs=lps, count=n)
        return results

    # ------------------------------------------------------------------ log-probabilities of generated tokens
    def _logprobs_on(self, n: int):
        """The current bank records the log-probability of every token it generates from now on, with at least `n` alternatives
        (`scoring.token_logprobs`): one more launch behind every pick.  The state is a buffer this engine allocates per bank on first
        use; the bank's decode graphs are re-captured once.  Sticky, like `_sampling_on`: later calls without logprobs= keep
        recording (`logprobs_off` ends it).  A process that never asks never gets here."""
        cur = self._lp_top.get(self._bank)
        if cur is not None and cur >= n:
            return                                                # the first n of more ranks are the n ranks: same rounds, same bits
        nbytes = int(self.L.aur_logprob_bytes(self.ctx, n))
        buf = self._lp_bufs.get(self._bank)
        if buf is None or buf.numel() < nbytes:
            torch.cuda.synchronize(self.dev)                      # queued steps may still write the buffer this one replaces
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        check(self.ctx, self.L.aur_logprob_enable(self.ctx, n, buf.data_ptr(), nbytes, self._stream()), "aur_logprob_enable")
        self._lp_bufs[self._bank], self._lp_top[self._bank] = buf, n

    def logprobs_off(self):
        """No bank records log-probabilities any more: the launches are those of an engine that never asked (the buffers are kept
        for the next request)."""
        bank = self._bank
        for b in sorted(self._lp_top):
            self.select_bank(b)
            check(self.ctx, self.L.aur_logprob_enable(self.ctx, 0, None, 0, self._stream()), "aur_logprob_enable")
            del self._lp_top[b]
        self.select_bank(bank)

    def token_logprob_state(self):
        """The current bank's records as numpy (synchronises): lens int32 [batch], token log-probabilities float32 [batch, max_new],
        top ids int32 / top log-probabilities float32 [batch, max_new, top_n].  Entries at or beyond a slot's length are 0 / (-1, 0)."""
        top = self._lp_top[self._bank]
        B, M = self._batch, self._max_new
        lens, lp = np.zeros(B, np.int32), np.zeros((B, M), np.float32)
        tid, tlp = np.zeros((B, M, top), np.int32), np.zeros((B, M, top), np.float32)
        check(self.ctx, self.L.aur_get_logprobs(self.ctx, lp.ctypes.data_as(C.c_void_p), tid.ctypes.data_as(C.c_void_p),
                                                tlp.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), self._stream()),
              "aur_get_logprobs")
        return lens, lp, tid, tlp

    def slot_collect_logprobs(self, slot0: int, nslots: int, lp_dev: torch.Tensor, top_ids_dev: torch.Tensor, top_lp_dev: torch.Tensor,
                              lens_dev: torch.Tensor):
        """Async device copy of the records of slots [slot0, slot0 + nslots) (`slot_collect`'s counterpart): lp_dev float32
        [nslots, max_new], top_ids_dev int32 / top_lp_dev float32 [nslots, max_new, top_n of the bank], lens_dev int32 [nslots]."""
        top = self._lp_top[self._bank]
        n = nslots * self._max_new
        assert lp_dev.dtype == torch.float32 and top_lp_dev.dtype == torch.float32 and top_ids_dev.dtype == torch.int32 and lens_dev.dtype == torch.int32
        assert all(t.is_cuda and t.is_contiguous() for t in (lp_dev, top_ids_dev, top_lp_dev, lens_dev))
        assert lp_dev.numel() >= n and top_ids_dev.numel() >= n * top and top_lp_dev.numel() >= n * top and lens_dev.numel() >= nslots
        check(self.ctx, self.L.aur_slot_collect_logprobs(self.ctx, slot0, nslots, lp_dev.data_ptr(), top_ids_dev.data_ptr(), top_lp_dev.data_ptr(),
                                                         lens_dev.data_ptr(), self._stream()), "aur_slot_collect_logprobs")

    def token_logprob_rows(self, logits: torch.Tensor, tokens, top_n: int = 0):
        """The kernel alone (aur_token_logprob_rows): logits fp32 [rows, vocab] on the device, one token per row (a list, or an int32
        device tensor) -> (log-probabilities float32 [rows], top ids int32 [rows, top_n], their log-probabilities float32
        [rows, top_n]) as numpy.  A token outside [0, vocab): (0, -1 .., 0 ..)."""
        top_n = check_logprobs(top_n)
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) == logits.shape[1]
        rows, vocab = logits.shape
        tg = tokens if torch.is_tensor(tokens) else torch.tensor([int(t) for t in tokens], dtype=torch.int32, device=self.dev)
        assert tg.dtype == torch.int32 and tg.is_cuda and tg.numel() >= rows
        lp = torch.empty(rows, dtype=torch.float32, device=self.dev)
        tid = torch.empty(rows, max(top_n, 1), dtype=torch.int32, device=self.dev)
        tlp = torch.empty(rows, max(top_n, 1), dtype=torch.float32, device=self.dev)
        check(self.ctx, self.L.aur_token_logprob_rows(self.ctx, logits.data_ptr(), rows, vocab, tg.data_ptr(), top_n, lp.data_ptr(),
                                                      tid.data_ptr(), tlp.data_ptr(), self._stream()), "aur_token_logprob_rows")
        torch.cuda.synchronize()
        return lp.cpu().numpy(), tid.cpu().numpy()[:, :top_n], tlp.cpu().numpy()[:, :top_n]

    # ------------------------------------------------------------------ attention over the prompt during decode
    def _attn_map_on(self, window: int, layers=None):
        """The current bank records, for every token it generates from now on, the attention of its decode step over keys
        [0, window) - mean over `layers` (None = all) and all heads, as `aurora_amd.attn_map` defines it: two more launches behind the
        QKV projection of every selected layer.  The state is a buffer this engine allocates per bank on first use; the bank's decode
        graphs are re-captured once and the front-end graphs dropped when the choice changes (they hold slot resets and commits, which
        clear the rows).  Sticky, like `_logprobs_on` (`attn_map_off` ends it).  A process that never asks never gets here."""
        want = (int(window), None if layers is None else tuple(layers))
        if self._am_on.get(self._bank) == want:
            return
        nbytes = int(self.L.aur_attn_map_bytes(self.ctx, want[0]))
        if nbytes < 0:
            raise ValueError(f"attn_map keys={want[0]} is not a multiple of 64 within the engine's context of {self.c.max_ctx}")
        self._drop_front_graphs()
        buf = self._am_bufs.get(self._bank)
        if buf is None or buf.numel() < nbytes:
            torch.cuda.synchronize(self.dev)                      # queued steps may still write the buffer this one replaces
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        check(self.ctx, self.L.aur_attn_map_enable(self.ctx, want[0], AM.layer_mask(want[1]), buf.data_ptr(), buf.numel(), self._stream()),
              "aur_attn_map_enable")
        self._am_bufs[self._bank], self._am_on[self._bank] = buf, want

    def attn_map_off(self):
        """No bank records attention any more: the launches are those of an engine that never asked (the buffers are kept for the
        next request)."""
        if not self._am_on:
            return
        self._drop_front_graphs()
        bank = self._bank
        for b in sorted(self._am_on):
            self.select_bank(b)
            check(self.ctx, self.L.aur_attn_map_enable(self.ctx, 0, 0, None, 0, self._stream()), "aur_attn_map_enable")
            del self._am_on[b]
        self.select_bank(bank)

    def attn_map_state(self) -> np.ndarray:
        """The current bank's records as numpy (synchronises): float32 [batch, max_new, window].  Row 0 of a slot and rows at or beyond
        its length are zeros."""
        W = self._am_on[self._bank][0]
        out = np.zeros((self._batch, self._max_new, W), np.float32)
        check(self.ctx, self.L.aur_get_attn_map(self.ctx, out.ctypes.data_as(C.c_void_p), self._stream()), "aur_get_attn_map")
        return out

    def slot_collect_attn_map(self, slot0: int, nslots: int, out_dev: torch.Tensor):
        """Async device copy of the records of slots [slot0, slot0 + nslots) (`slot_collect`'s counterpart): out_dev float32
        [nslots, max_new, window of the bank]."""
        W = self._am_on[self._bank][0]
        assert out_dev.dtype == torch.float32 and out_dev.is_cuda and out_dev.is_contiguous() and out_dev.numel() >= nslots * self._max_new * W
        check(self.ctx, self.L.aur_slot_collect_attn_map(self.ctx, slot0, nslots, out_dev.data_ptr(), self._stream()), "aur_slot_collect_attn_map")

    def attn_map_rows(self, x: torch.Tensor, w_packed: torch.Tensor, pos, window: int, *, rope: bool = False) -> torch.Tensor:
        """The recorder's kernels alone (aur_attn_map_rows), beside `attn_decode_rows` and with its arguments: one decode step's QKV
        write on caller rows x [B, kx], then the attention of row b over keys [0, window) of KV sequence b at position pos[b] - one
        layer, mean over all heads.  Returns float32 [B, window] on the device."""
        xh = self._h(x)
        B, kx = xh.shape
        pos_t = self._i32_arg(pos, B, "pos")
        scratch = torch.empty(max(int(self.L.aur_attn_map_rows_scratch_bytes(self.ctx, kx, int(window))), 256), dtype=torch.uint8, device=self.dev)
        out = torch.full((B, int(window)), float("nan"), dtype=torch.float32, device=self.dev)
        check(self.ctx, self.L.aur_attn_map_rows(self.ctx, xh.data_ptr(), B, kx, w_packed.data_ptr(), w_packed.numel() // kx, pos_t.data_ptr(),
                                                 int(rope), scratch.data_ptr(), scratch.numel(), int(window), out.data_ptr(), self._stream()),
              "aur_attn_map_rows")
        torch.cuda.synchronize()
        return out

    def _attn_map_request(self, attn_map, prompt_len: Optional[int]):
        """`attn_map=` of a generation call -> the window it records with (None: not asked), the bank switched on.  prompt_len None
        (a stream of clips whose prompts differ): keys=None is the engine's whole context."""
        if attn_map is None:
            return None
        am = AM.check_attn_map(attn_map, self.l["num_hidden_layers"])
        W = am[0] if am[0] is not None else AM.window_for(self.c.max_ctx if prompt_len is None else prompt_len)
        self._attn_map_on(W, am[1])
        return W

    def _outputs(self, lpn, amw, count: Optional[int] = None):
        """`outputs(lpn)`, and with attn_map= asked a dict per slot (an ids list becomes dict(ids=...)) that also holds attn_map
        float32 [n_tokens, window]"""
        out = self.outputs(lpn, count)
        if amw is None:
            return out
        state = self.attn_map_state()
        res = []
        for b, r in enumerate(out):
            r = dict(r) if isinstance(r, dict) else dict(ids=r)
            r["attn_map"] = state[b, :len(r["ids"])].copy()
            res.append(r)
        return res

    # ------------------------------------------------------------------ sampling
    def _sampling_on(self):
        """The first sampling request switches the ctx's token pick to sample_advance_kernel (decode graphs are re-captured once);
        slots whose temperature is 0 keep the greedy rule bit for bit.  A process that never samples never gets here."""
        if not self._sampling_mode:
            self._drop_front_graphs()
            self.set_option("sampling", 1)
            self._sampling_mode = True

    def _drop_front_graphs(self):
        """Before an option that changes which kernels a prefill / commit launches is flipped: no front-end graph captured under
        the old setting is replayed under the new one (today's graphs hold the stage only - the pick is the eager commit's - so this
        is the guard for one that captures a commit, as `graph_capture` allows)."""
        for fg in self._front_graphs.values():
            if getattr(fg, "_last", None) is not None:
                fg._last.synchronize()
            fg.close()
        self._front_graphs = {}

    # ------------------------------------------------------------------ logit rules
    def _rules_on(self):
        """The first request with non-neutral logit rules brackets the ctx's token pick with logit_rules_apply_kernel /
        logit_rules_restore_kernel (decode graphs are re-captured once, the side lists are allocated); slots whose record is
        neutral are not touched.  Sticky, like `_sampling_on`.  A process that never asks never gets here."""
        if not self._rules_mode:
            self._drop_front_graphs()
            self.set_option("logit_rules", 1)
            self._rules_mode = True

    def slot_logit_rules(self, slot0: int, recs: np.ndarray):
        """Give slots [slot0, slot0 + len(recs)) of the current bank their aur_logit_rules records (`logit_rules.records`): staged
        in device memory and copied into the bank when the stream gets there - before the prefill / commit that picks the first
        token.  The history the rules see is the slot's generated tokens, not its prompt."""
        recs = np.ascontiguousarray(recs, dtype=LR.RECORD)
        n = len(recs)
        if n < 1 or slot0 < 0 or slot0 + n > self.max_batch:
            raise ValueError(f"slots [{slot0}, {slot0 + n}) outside an engine of {self.max_batch} slots")
        if self._rules_stage is None:
            self._rules_stage = torch.zeros(2 * self.max_batch, LR.RECORD.itemsize, dtype=torch.uint8, device=self.dev)
        row0 = self._bank * self.max_batch + slot0
        dst = self._rules_stage[row0: row0 + n]
        dst.copy_(torch.from_numpy(recs.view(np.uint8).reshape(n, LR.RECORD.itemsize).copy()))     # torch's current stream: _stream() orders ours behind it
        check(self.ctx, self.L.aur_slot_logit_rules(self.ctx, slot0, n, dst.data_ptr(), self._stream()), "aur_slot_logit_rules")

    def logit_rules_rows(self, logits: torch.Tensor, histories: Sequence[Sequence[int]], recs: np.ndarray, eos_id: Optional[int],
                         restore: bool = False, ids_stride: Optional[int] = None) -> torch.Tensor:
        """The rule kernels alone (aur_logit_rules_rows) on a copy of `logits` (fp32 [rows, vocab] on the device): one generated
        history and one aur_logit_rules record per row -> the processed rows (restore=False) or the rows after apply + restore
        (restore=True), on the device.  ids_stride: the row stride of the history buffer (default: the longest history, at least 1)."""
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.is_contiguous() and logits.dim() == 2
        rows, vocab = logits.shape
        recs = np.ascontiguousarray(recs, dtype=LR.RECORD)
        assert len(recs) == rows and len(histories) == rows
        stride = max([1] + [len(h) for h in histories]) if ids_stride is None else int(ids_stride)
        assert stride >= 1 and all(len(h) <= stride for h in histories)
        ids = np.zeros((rows, stride), np.int32)
        for i, h in enumerate(histories):
            ids[i, :len(h)] = np.asarray(h, np.int32)
        ids_d = torch.from_numpy(ids).to(self.dev)
        lens_d = torch.tensor([len(h) for h in histories], dtype=torch.int32, device=self.dev)
        rec_d = torch.from_numpy(recs.view(np.uint8).reshape(rows, LR.RECORD.itemsize).copy()).to(self.dev)
        out = logits.clone()
        check(self.ctx, self.L.aur_logit_rules_rows(self.ctx, out.data_ptr(), rows, vocab, ids_d.data_ptr(), stride, lens_d.data_ptr(),
                                                    rec_d.data_ptr(), -1 if eos_id is None else int(eos_id), 1 if restore else 0,
                                                    self._stream()), "aur_logit_rules_rows")
        torch.cuda.synchronize()
        return out

    def _begin_rules(self, rules: Optional[dict], B: int):
        """After begin_batch (which makes every slot neutral): the records of slots [0, B) for a call with logit rules."""
        if rules is not None:
            self.slot_logit_rules(0, LR.records(rules, B))

    # ------------------------------------------------------------------ classifier-free guidance
    def _guidance_on(self):
        """The first guided request puts guidance_apply_kernel / guidance_restore_kernel around the ctx's token pick and
        guidance_follow_kernel behind the stop check (decode graphs are re-captured once, the banks' records and save buffers are
        allocated); slots whose record is neutral are not touched.  Sticky, like `_rules_on`.  A process that never asks never
        gets here."""
        if not self._guid_mode:
            self._drop_front_graphs()
            self.set_option("guidance", 1)
            self._guid_mode = True

    def slot_guidance(self, slot0: int, recs: np.ndarray):
        """Give slots [slot0, slot0 + len(recs)) of the current bank their aur_guidance records (`guidance.records`): staged in
        device memory and copied into the bank when the stream gets there - before the prefill / commit that picks the first token.
        A leader's record names its partner; prefill the partner first, its row is what the leader's first pick contrasts with."""
        recs = np.ascontiguousarray(recs, dtype=GD.RECORD)
        n = len(recs)
        if n < 1 or slot0 < 0 or slot0 + n > self.max_batch:
            raise ValueError(f"slots [{slot0}, {slot0 + n}) outside an engine of {self.max_batch} slots")
        if self._guid_stage is None:
            self._guid_stage = torch.zeros(2 * self.max_batch, GD.RECORD.itemsize, dtype=torch.uint8, device=self.dev)
        row0 = self._bank * self.max_batch + slot0
        dst = self._guid_stage[row0: row0 + n]
        dst.copy_(torch.from_numpy(recs.view(np.uint8).reshape(n, GD.RECORD.itemsize).copy()))     # torch's current stream: _stream() orders ours behind it
        check(self.ctx, self.L.aur_slot_guidance(self.ctx, slot0, n, dst.data_ptr(), self._stream()), "aur_slot_guidance")

    def guidance_rows(self, logits: torch.Tensor, recs: np.ndarray, restore: bool = False, b0: int = 0, nb: Optional[int] = None):
        """The guidance kernels alone (aur_guidance_rows) on a copy of `logits` (fp32 [rows, vocab] on the device), one aur_guidance
        record per row, partners being rows of the same buffer; the kernels see rows [b0, b0 + nb) alone (default: all), whose
        partners must lie among them -> (rows, save) on the device: the whole buffer and the whole save buffer behind
        guidance_apply_kernel (restore=False) or behind apply + restore (restore=True).  The save buffer starts as NaN with the bit
        pattern 0x7fc0beef."""
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.dim() == 2
        rows, vocab = logits.shape
        recs = np.ascontiguousarray(recs, dtype=GD.RECORD)
        nb = rows - b0 if nb is None else int(nb)
        assert len(recs) == rows and 0 <= b0 and nb >= 1 and b0 + nb <= rows
        sub = recs[b0:b0 + nb].copy()
        lead = (sub["scale"] > 0) & (sub["scale"] != 1) & np.isfinite(sub["scale"])
        assert ((sub["partner"][lead] >= b0) & (sub["partner"][lead] < b0 + nb)).all(), "a partner outside the launched rows"
        sub["partner"][lead] -= b0
        rec_d = torch.from_numpy(sub.view(np.uint8).reshape(nb, GD.RECORD.itemsize).copy()).to(self.dev)
        out = logits.clone().contiguous()
        save = torch.full((rows, vocab), 0x7fc0beef, dtype=torch.int32, device=self.dev).view(torch.float32)
        torch.cuda.synchronize()
        for mode in ((0, 1) if restore else (0,)):
            check(self.ctx, self.L.aur_guidance_rows(self.ctx, out[b0:].data_ptr(), nb, vocab, rec_d.data_ptr(), save[b0:].data_ptr(),
                                                     mode, self._stream()), "aur_guidance_rows")
        torch.cuda.synchronize()
        return out, save

    def _begin_guidance(self, gd: Optional[dict], pairs, count: int):
        """After begin_batch (which makes every slot neutral): the records of slots [0, count) for a guided call."""
        if gd is not None:
            self.slot_guidance(0, GD.records(gd["scale"], pairs, count))

    # ------------------------------------------------------------------ stop conditions
    def set_stop_vocab(self, table):
        """Hand the ctx the bytes every vocabulary entry decodes to: `stopping.token_bytes(tokenizer)`, built once per tokenizer -
        (offsets int32 [V + 1], bytes uint8).  Needed before any request with stop strings; None takes it back.  Decode graphs that
        froze the previous table are re-captured."""
        if table is None:
            check(self.ctx, self.L.aur_stop_vocab(self.ctx, None, None, 0, 0), "aur_stop_vocab")
            self._stop_table = self._stop_table_dev = None
            return
        off = np.ascontiguousarray(table[0], np.int32)
        data = np.ascontiguousarray(table[1], np.uint8)
        if off.ndim != 1 or len(off) < 2 or data.ndim != 1 or len(data) < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] > len(data):
            raise ValueError("stop vocabulary: offsets int32 [V + 1], ascending from 0, into bytes uint8")
        if int(np.diff(off).max()) > ST.MAX_TOKEN_BYTES:
            raise ValueError(f"stop vocabulary: a token of more than {ST.MAX_TOKEN_BYTES} bytes")
        dev = (torch.from_numpy(off).to(self.dev), torch.from_numpy(data).to(self.dev))
        torch.cuda.synchronize()
        check(self.ctx, self.L.aur_stop_vocab(self.ctx, dev[0].data_ptr(), dev[1].data_ptr(), len(off) - 1, len(data)), "aur_stop_vocab")
        self._stop_table, self._stop_table_dev = (off, data), dev

    def _stop_on(self):
        """The first request with a non-neutral stop record puts stop_check_kernel behind the ctx's token pick (decode graphs are
        re-captured once, the banks' records are allocated); slots whose record is neutral stop on the EOS and the batch's limit
        alone, as before.  Sticky, like `_sampling_on`.  A process that never asks never gets here."""
        if not self._stop_mode:
            self._drop_front_graphs()
            self.set_option("stop_rules", 1)
            self._stop_mode = True

    def _stop_records(self, stop, count: int, max_new_tokens: int):
        """A call's `stop=` for `count` sequences -> validated records, or None (then the call is one without the argument)."""
        return ST.per_sequence(stop, count, max_new_tokens, self._stop_table)

    def slot_stop(self, slot0: int, recs: np.ndarray):
        """Give slots [slot0, slot0 + len(recs)) of the current bank their aur_stop_rules records (`stopping.records`): staged in
        device memory and copied into the bank when the stream gets there - before the prefill / commit that picks the first token."""
        recs = np.ascontiguousarray(recs, dtype=ST.RECORD)
        n = len(recs)
        if n < 1 or slot0 < 0 or slot0 + n > self.max_batch:
            raise ValueError(f"slots [{slot0}, {slot0 + n}) outside an engine of {self.max_batch} slots")
        if self._stop_stage is None:
            self._stop_stage = torch.zeros(2 * self.max_batch, ST.RECORD.itemsize, dtype=torch.uint8, device=self.dev)
        row0 = self._bank * self.max_batch + slot0
        dst = self._stop_stage[row0: row0 + n]
        dst.copy_(torch.from_numpy(recs.view(np.uint8).reshape(n, ST.RECORD.itemsize).copy()))     # torch's current stream: _stream() orders ours behind it
        check(self.ctx, self.L.aur_slot_stop(self.ctx, slot0, n, dst.data_ptr(), self._stream()), "aur_slot_stop")

    def _begin_stop(self, stops, B: int):
        """After begin_batch (which makes every slot neutral): the records of slots [0, B) for a call with stop records."""
        if stops is not None:
            self.slot_stop(0, ST.records(stops))

    def stop_rows(self, histories: Sequence[Sequence[int]], recs: np.ndarray, batch_max_new: int, finished=None, table=None,
                  ids_stride: Optional[int] = None) -> np.ndarray:
        """stop_check_kernel alone (aur_stop_rows): one generated history and one aur_stop_rules record per row -> the rows'
        `finished` flags (numpy int32) behind the kernel.  finished: the flags before it (default: none set); a row whose flag is
        set is skipped.  table: (offsets, bytes) as `stopping.token_bytes` gives it, or None (no string matches).  ids_stride: the
        row stride of the history buffer (default: the longest history, at least 1)."""
        rows = len(histories)
        recs = np.ascontiguousarray(recs, dtype=ST.RECORD)
        assert rows >= 1 and len(recs) == rows
        stride = max([1] + [len(h) for h in histories]) if ids_stride is None else int(ids_stride)
        assert stride >= 1 and all(len(h) <= stride for h in histories)
        ids = np.zeros((rows, stride), np.int32)
        for i, h in enumerate(histories):
            ids[i, :len(h)] = np.asarray(h, np.int64).astype(np.int32)
        ids_d = torch.from_numpy(ids).to(self.dev)
        lens_d = torch.tensor([len(h) for h in histories], dtype=torch.int32, device=self.dev)
        rec_d = torch.from_numpy(recs.view(np.uint8).reshape(rows, ST.RECORD.itemsize).copy()).to(self.dev)
        fin = np.zeros(rows, np.int32) if finished is None else np.ascontiguousarray(finished, np.int32).copy()
        assert len(fin) == rows
        fin_d = torch.from_numpy(fin).to(self.dev)
        off_p = data_p = None
        V = nbytes = 0
        if table is not None:
            off_d = torch.from_numpy(np.ascontiguousarray(table[0], np.int32)).to(self.dev)
            data_d = torch.from_numpy(np.ascontiguousarray(table[1], np.uint8)).to(self.dev)
            off_p, data_p, V, nbytes = off_d.data_ptr(), data_d.data_ptr(), off_d.numel() - 1, data_d.numel()
        torch.cuda.synchronize()
        check(self.ctx, self.L.aur_stop_rows(self.ctx, rows, ids_d.data_ptr(), stride, lens_d.data_ptr(), rec_d.data_ptr(), fin_d.data_ptr(),
                                             int(batch_max_new), off_p, data_p, V, nbytes, self._stream()), "aur_stop_rows")
        torch.cuda.synchronize()
        return fin_d.cpu().numpy()

    def slot_sampling(self, slot0: int, recs: np.ndarray):
        """Give slots [slot0, slot0 + len(recs)) of the current bank their aur_sampling records (`sampling.records`): staged in
        device memory and copied into the bank when the stream gets there - before the prefill / commit that picks the first token."""
        recs = np.ascontiguousarray(recs, dtype=S.RECORD)
        n = len(recs)
        if n < 1 or slot0 < 0 or slot0 + n > self.max_batch:
            raise ValueError(f"slots [{slot0}, {slot0 + n}) outside an engine of {self.max_batch} slots")
        if self._samp_stage is None:
            self._samp_stage = torch.zeros(2 * self.max_batch, S.RECORD.itemsize, dtype=torch.uint8, device=self.dev)
        row0 = self._bank * self.max_batch + slot0
        dst = self._samp_stage[row0: row0 + n]
        dst.copy_(torch.from_numpy(recs.view(np.uint8).reshape(n, S.RECORD.itemsize).copy()))      # torch's current stream: _stream() orders ours behind it
        check(self.ctx, self.L.aur_slot_sampling(self.ctx, slot0, n, dst.data_ptr(), self._stream()), "aur_slot_sampling")

    def _begin_sampled(self, samp: Optional[dict], streams, B: int):
        """After begin_batch (which makes every slot greedy): the records of slots [0, B) for a sampling call."""
        if samp is None:
            return
        streams = list(range(B)) if streams is None else [int(x) for x in streams]
        if len(streams) != B:
            raise ValueError(f"{len(streams)} streams for {B} sequences")
        self.slot_sampling(0, S.records(samp, streams))

    def sample_rows(self, logits: torch.Tensor, recs: np.ndarray, n: Sequence[int]):
        """The sampled pick alone (aur_sample_rows): logits fp32 [rows, vocab] on the device, one aur_sampling record and one token
        index per row -> (tokens, kept-set sizes) as numpy int32."""
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.is_contiguous() and logits.dim() == 2
        rows, vocab = logits.shape
        recs = np.ascontiguousarray(recs, dtype=S.RECORD)
        assert len(recs) == rows and len(n) == rows
        prm = torch.from_numpy(recs.view(np.uint8).reshape(rows, S.RECORD.itemsize).copy()).to(self.dev)
        nd = torch.tensor([int(x) for x in n], dtype=torch.int32, device=self.dev)
        tok = torch.empty(rows, dtype=torch.int32, device=self.dev)
        kept = torch.empty(rows, dtype=torch.int32, device=self.dev)
        check(self.ctx, self.L.aur_sample_rows(self.ctx, logits.data_ptr(), rows, vocab, prm.data_ptr(), nd.data_ptr(), tok.data_ptr(),
                                               kept.data_ptr(), self._stream()), "aur_sample_rows")
        torch.cuda.synchronize()
        return tok.cpu().numpy(), kept.cpu().numpy()

    def generate(self, embeds_list, seq_lens, max_new_tokens: int, eos_id: Optional[int] = 2, check_every: int = 32,
                 sampling: Optional[dict] = None, streams: Optional[Sequence[int]] = None, logprobs: Optional[int] = None,
                 logit_rules: Optional[dict] = None, stop=None, attn_map: Optional[dict] = None, guidance: Optional[dict] = None):
        """Generation for a batch of already-spliced prefixes (one KV slot per sequence): greedy, or with
        sampling=dict(temperature, top_k, top_p, seed) drawn as `aurora_amd.sampling` defines it; `streams` (default range(B)) are
        the sequences' request indices - a sequence's ids depend on (seed, its stream), not on its slot or its neighbours.
        logprobs=n (0 .. 8): each result is a dict - ids, token_logprobs float32 [len], top_ids int32 [len, n], top_logprobs float32
        [len, n] - as `scoring.token_logprobs` defines them: under the model's unmodified distribution, whatever `sampling` says;
        the ids are the same.  None: the list of ids, and no extra work.
        logit_rules=dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0), one dict for the call: transformers'
        three processors on the raw row ahead of the pick, greedy or sampled, as `aurora_amd.logit_rules` defines them - over the
        tokens GENERATED so far, never the prompt (what `generate(inputs_embeds=...)` gives the reference).  Log-probabilities stay
        those of the unmodified row.  None or all-neutral values: exactly the path of a call without the argument.
        stop=dict(token_ids=(), strings=(), max_new_tokens=0) for every sequence, or a list with one dict or None per sequence: a
        sequence also ends behind a token that is one of its stop ids, behind one whose bytes complete one of its stop strings
        (`set_stop_vocab` first), or when it holds its own max_new_tokens - decided on the device behind every pick, as
        `aurora_amd.stopping` defines it; the token that stops it stays in the output and `stopping.finish_reason` names the reason
        from the ids.  None or all-neutral records: exactly the path of a call without the argument.
        attn_map=dict(keys=W or None, layers=None or a list): each result is a dict that also holds attn_map float32 [len, W] - row i
        the attention of the decode step that picked token i over keys [0, W) of its context, mean over the layers (None = all) and
        all heads, as `aurora_amd.attn_map` defines it; row 0 (the prefill's token) is zeros.  keys=None: the longest prompt rounded
        up to 64.  The ids are the same.  None: no extra work.
        guidance=dict(scale=g, negative=[(embeds, seq_len), ...]), one negative prefix per sequence: classifier-free guidance as
        `aurora_amd.guidance` defines it.  Sequence i decodes in slot i, its negative in slot B + i, in lock-step; ahead of every pick
        - and of the logit rules - row i becomes g * (log_softmax(row i) - log_softmax(row B + i)) + log_softmax(row B + i), and the
        token picked from it is appended to both.  A guided call needs 2 B <= max_batch.  The results are the B sequences' alone, in
        every form; log-probabilities stay those of the model's conditional row.  None, or a scale of None / 1: exactly the path of
        a call without the argument."""
        lpn = check_logprobs(logprobs)
        amw = None if attn_map is None else self._attn_map_request(attn_map, max(seq_lens) if len(seq_lens) else 1)
        B = len(embeds_list)
        gd = GD.check_guidance(guidance)
        pairs = None
        if gd is not None:
            negs = gd.get("negative")
            if negs is None or len(negs) != B:
                raise ValueError(f"guidance: `negative` must hold one (embeds, seq_len) per sequence ({B})")
            pairs = GD.pair_slots(B, self.max_batch)
        samp = S.check_sampling(sampling)
        rules = LR.check_logit_rules(logit_rules)
        stops = None if stop is None else self._stop_records(stop, B, max_new_tokens)
        if samp is not None:
            self._sampling_on()
        if rules is not None:
            self._rules_on()
        if stops is not None:
            self._stop_on()
        if lpn is not None:
            self._logprobs_on(lpn)
        if gd is not None:
            self._guidance_on()
        self.begin_batch(B if gd is None else 2 * B, max_new_tokens, eos_id)
        self._begin_sampled(samp, streams, B)
        self._begin_rules(rules, B)
        self._begin_stop(stops, B)
        if gd is not None:                                        # the partners first: a leader's first pick reads its partner's row
            self._begin_guidance(gd, pairs, 2 * B)
            for lead, part in pairs:
                self.prefill(part, negs[lead][0], negs[lead][1])
        for b in range(B):
            self.prefill(b, embeds_list[b], seq_lens[b])
        may_end = eos_id is not None or stops is not None
        done = 1
        while done < max_new_tokens:
            n = min(check_every, max_new_tokens - done) if may_end else max_new_tokens - done
            self.decode(n)
            done += n
            if may_end and self.unfinished() == 0:
                break
        return (self.outputs(lpn, B) if amw is None else self._outputs(lpn, amw, B))

    def _negative_ids(self, gd: dict, prompts: Sequence[Sequence[int]]) -> List[List[int]]:
        """The negative prompt of every request of a guided caption call.  negative_ids None: the request's own prompt without its
        image markers (the language prior alone); one list of ids: that prompt for every request; a list of lists: one each."""
        neg = gd.get("negative_ids")
        n = len(prompts)
        if neg is None:
            out = [[int(t) for t in ids if t != IMAGE_TOKEN_INDEX] for ids in prompts]
        elif len(neg) and isinstance(neg[0], (list, tuple, np.ndarray)) or torch.is_tensor(neg) and neg.dim() == 2:
            if len(neg) != n:
                raise ValueError(f"guidance: {len(neg)} negative prompts for {n} requests")
            out = [[int(t) for t in ids] for ids in neg]
        else:
            out = [[int(t) for t in neg] for _ in range(n)]
        if any(len(ids) < 1 for ids in out):
            raise ValueError("guidance: an empty negative prompt")
        return out

    def _negative_embeds(self, vis: torch.Tensor, neg_ids: Sequence[int]):
        """A negative prompt's spliced prefix: markers it keeps take the SAME kept visual rows (no second ViT pass); without markers
        it is a text-only splice (zero frames, zero visual rows)."""
        if any(t == IMAGE_TOKEN_INDEX for t in neg_ids):
            return self.project_splice(vis, neg_ids)
        return self.text_embeds(neg_ids)

    def text_embeds(self, ids: Sequence[int]):
        """Text ids through the embedding table alone -> (embeds [L_pad, d] fp16, seq_len): the splice of a prompt without frames
        (image markers among the ids are dropped, as `splice_rows` drops markers beyond the number of frames)."""
        plan = self.splice_plan([int(t) for t in ids], 0, 0)
        if plan["seq_len"] < 1:
            raise ValueError("a prompt without text tokens")
        none = torch.empty(0, 0, self.v["hidden_size"], dtype=torch.float16, device=self.dev)
        return self.project_splice(none, plan=plan)

    def _caption_batch_guided(self, clips, token_kept_ratio, max_new_tokens, eos_id, check_every, sampling, streams, share, logprobs,
                              logit_rules, stop, attn_map, gd):
        """`caption_batch` under guidance: every clip's prefix and its negative's, then `generate`.  Clips with equal non-None share
        keys and equal shapes run the ViT once; their KV is not shared."""
        B = len(clips)
        GD.pair_slots(B, self.max_batch)
        if share is not None and len(share) != B:
            raise ValueError(f"{len(share)} share keys for {B} clips")
        negs = self._negative_ids(gd, [ids for _, ids in clips])
        vis_of, embs, lens, nemb = {}, [], [], []
        for i, (px, ids) in enumerate(clips):
            key = None if share is None or share[i] is None else (share[i], tuple(px.shape))
            vis = vis_of.get(key) if key is not None else None
            if vis is None:
                vis = self.vit_encode(px, self.tome_r(token_kept_ratio, px.shape[-2], px.shape[-1]))
                if key is not None:
                    vis_of[key] = vis
            emb, L = self.project_splice(vis, ids)
            embs.append(emb)
            lens.append(L)
            nemb.append(self._negative_embeds(vis, negs[i]))
        return self.generate(embs, lens, max_new_tokens, eos_id, check_every, sampling=sampling, streams=streams, logprobs=logprobs,
                             logit_rules=logit_rules, **({} if stop is None else dict(stop=stop)),
                             **({} if attn_map is None else dict(attn_map=attn_map)), guidance=dict(scale=gd["scale"], negative=nemb))

    def caption_ids(self, pixels: torch.Tensor, input_ids: Sequence[int], token_kept_ratio: float, max_new_tokens: int,
                    eos_id: Optional[int] = 2, sampling: Optional[dict] = None, stream: int = 0, logprobs: Optional[int] = None,
                    logit_rules: Optional[dict] = None, stop: Optional[dict] = None, attn_map: Optional[dict] = None,
                    guidance: Optional[dict] = None):
        """Whole path for one clip: the call sequence of inference.py:87-96.  sampling / stream / logprobs / logit_rules / stop /
        attn_map: as in `generate`.  guidance=dict(scale=g, negative_ids=None | ids): as in `caption_batch`."""
        gd = GD.check_guidance(guidance)
        if gd is not None:
            return self.caption_batch([(pixels, input_ids)], token_kept_ratio, max_new_tokens, eos_id, sampling=sampling, streams=[stream],
                                      logprobs=logprobs, logit_rules=logit_rules, stop=stop, attn_map=attn_map, guidance=gd)[0]
        check_logprobs(logprobs)
        if attn_map is not None:
            AM.check_attn_map(attn_map, self.l["num_hidden_layers"])
        LR.check_logit_rules(logit_rules)
        if stop is not None:
            self._stop_records(stop, 1, max_new_tokens)
        r = self.tome_r(token_kept_ratio, pixels.shape[-2], pixels.shape[-1])
        vis = self.vit_encode(pixels, r)
        emb, L = self.project_splice(vis, input_ids)
        return self.generate([emb], [L], max_new_tokens, eos_id, sampling=sampling, streams=[stream], logprobs=logprobs,
                             logit_rules=logit_rules, **({} if stop is None else dict(stop=stop)),
                             **({} if attn_map is None else dict(attn_map=attn_map)))[0]

    def caption_batch(self, clips: Sequence[Tuple[torch.Tensor, Sequence[int]]], token_kept_ratio: float, max_new_tokens: int,
                      eos_id: Optional[int] = 2, prefill_group: int = 8, check_every: int = 32, sampling: Optional[dict] = None,
                      streams: Optional[Sequence[int]] = None, share: Optional[Sequence] = None, logprobs: Optional[int] = None,
                      logit_rules: Optional[dict] = None, stop=None, attn_map: Optional[dict] = None, guidance: Optional[dict] = None):
        """Whole path for up to max_batch clips at once: (pixel_values [f, C, H, W], input_ids with -200 markers) each.
        Clips may differ in frame count and prompt; neighbours whose spliced length is equal share one prefill pass - with
        `prompt_bucket`, neighbours whose lengths round up to the same multiple of the bucket (`prefill_groups`).
        Every kernel on the path is batch-invariant, so each clip gets exactly the ids it gets when captioned alone.
        sampling=dict(temperature, top_k, top_p, seed): sampled captions; clip i draws with stream streams[i] (default: i).
        share: one hashable key per clip, or None.  Clips with equal non-None keys are the same visual input (the caller's word:
        several prompts about one video).  The first clip of a key is prefilled as always; each later one runs no ViT - its own plan
        is spliced over the first clip's kept visual rows -, takes the whole KV pages the two prompts have in common from the first
        clip's slot (`kv_copy_prefix`) and prefills only its remaining rows, neighbouring siblings in one pass (`extend_batch`).  A
        sibling whose prompt shares less than a page with the first clip's, or diverges from it before the visual rows end, takes the
        unshared path.  The same ids either way; share=None is exactly the path above.
        logprobs=n: a dict per clip instead of its ids, as in `generate`.
        logit_rules: one dict for every clip of the call, as in `generate` (each clip's own generated tokens are its history).
        stop: one dict for every clip, or a list with one dict or None per clip, as in `generate`; siblings get theirs like any clip.
        attn_map: as in `generate` - a dict per clip with its attn_map; keys=None is the longest spliced prompt rounded up to 64.
        guidance=dict(scale=g, negative_ids=None | ids | [ids, ...]): classifier-free guidance as in `generate`, at most
        max_batch // 2 clips.  negative_ids None: each clip's own prompt without its image markers - a text-only prefix, the language
        prior alone; a negative that keeps its markers is spliced over the clip's kept visual rows (no second ViT pass)."""
        gd = GD.check_guidance(guidance)
        if gd is not None:
            return self._caption_batch_guided(clips, token_kept_ratio, max_new_tokens, eos_id, check_every, sampling, streams, share,
                                              logprobs, logit_rules, stop, attn_map, gd)
        lpn = check_logprobs(logprobs)
        if attn_map is not None:
            AM.check_attn_map(attn_map, self.l["num_hidden_layers"])
        B = len(clips)
        samp = S.check_sampling(sampling)
        rules = LR.check_logit_rules(logit_rules)
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"{B} clips for an engine built with max_batch={self.max_batch}")
        stops = None if stop is None else self._stop_records(stop, B, max_new_tokens)
        if share is not None and len(share) != B:
            raise ValueError(f"{len(share)} share keys for {B} clips")
        d = self.l["hidden_size"]
        rs, plans = [], []
        for px, ids in clips:
            r = self.tome_r(token_kept_ratio, px.shape[-2], px.shape[-1])
            t0 = (px.shape[-2] // self.v["patch_size"]) * (px.shape[-1] // self.v["patch_size"]) + 1     # as vit_encode counts them
            rs.append(r)
            plans.append(self.splice_plan(ids, px.shape[0], tokens_at_layer(t0, r, self.v["num_hidden_layers"] - 1) - 1))
        # siblings: clip -> (first clip of its key, fork position); everything else is a run of clips prefilled as always
        child, first = {}, {}
        for i, key in enumerate(share if share is not None else ()):
            if key is None:
                continue
            p = first.setdefault(key, i)
            if p != i and clips[p][0].shape == clips[i][0].shape:
                fork = share_fork(plans[p], plans[i])
                if fork > 0:
                    child[i] = (p, fork)
        keep_vis = {p for p, _ in child.values()}
        vis_of = {}
        if samp is not None:
            self._sampling_on()
        if rules is not None:
            self._rules_on()
        if stops is not None:
            self._stop_on()
        if lpn is not None:
            self._logprobs_on(lpn)
        amw = None if attn_map is None else self._attn_map_request(attn_map, max(p["seq_len"] for p in plans))
        self.begin_batch(B, max_new_tokens, eos_id)
        self._begin_sampled(samp, streams, B)
        self._begin_rules(rules, B)
        self._begin_stop(stops, B)
        runs, b0 = [], 0                                          # maximal runs of neighbouring clips that are nobody's sibling
        for i in range(B + 1):
            if i == B or i in child:
                if i > b0:
                    runs.append((b0, i))
                b0 = i + 1
        for r0, r1 in runs:
            for b, g, stride in prefill_groups([p["seq_len"] for p in plans[r0:r1]], prefill_group, self.prompt_bucket):
                b += r0
                lens = [plans[b + i]["seq_len"] for i in range(g)]
                mixed = len(set(lens)) > 1                        # only with a bucket: lengths go to the device, rows beyond them are don't-care
                L = stride if mixed else lens[0]
                Lp = _rup(L, 32)
                buf = torch.empty(g * Lp, d, dtype=torch.float16, device=self.dev)
                for i in range(g):
                    vis = self.vit_encode(clips[b + i][0], rs[b + i])
                    if b + i in keep_vis:
                        vis_of[b + i] = vis
                    self.project_splice(vis, out=buf[i * Lp:(i + 1) * Lp], plan=plans[b + i])
                self.prefill_batch(b, g, buf, L, seq_lens=lens if mixed else None)
        i = 0
        while i < B:                                              # neighbouring siblings of one (first clip, fork): one copy, one pass
            if i not in child:
                i += 1
                continue
            g = 1
            while i + g in child and child[i + g] == child[i] and g < prefill_group:
                g += 1
            p, fork = child[i]
            new = [plans[i + j]["seq_len"] - fork for j in range(g)]
            stride = _rup(max(new), 32)
            buf = torch.empty(g * stride, d, dtype=torch.float16, device=self.dev)
            for j in range(g):
                self._extend_rows(vis_of[p], plans[i + j], fork, buf[j * stride:(j + 1) * stride])
            self.kv_copy_prefix(p, i, g, fork)
            self.extend_batch(i, g, buf, fork, stride, new)
            i += g
        may_end = eos_id is not None or stops is not None
        done = 1
        while done < max_new_tokens:
            n = min(check_every, max_new_tokens - done) if may_end else max_new_tokens - done
            self.decode(n)
            done += n
            if may_end and self.unfinished() == 0:
                break
        return (self.outputs(lpn) if amw is None else self._outputs(lpn, amw))

    def caption_prompts(self, pixels: torch.Tensor, list_of_input_ids: Sequence[Sequence[int]], token_kept_ratio: float, max_new_tokens: int,
                        eos_id: Optional[int] = 2, sampling: Optional[dict] = None, streams: Optional[Sequence[int]] = None,
                        logprobs: Optional[int] = None, logit_rules: Optional[dict] = None, stop=None, attn_map: Optional[dict] = None,
                        guidance: Optional[dict] = None):
        """One clip, several prompts: `caption_batch` over (pixels, ids) for every prompt with one share key, in chunks of max_batch
        (the ViT runs once per chunk).  Ids in prompt order, each what `caption_ids(pixels, ids)` gives.  logprobs / logit_rules: as
        in `generate`; stop: one dict for every prompt, or a list with one dict or None per prompt; attn_map: as in `caption_batch`,
        per chunk.  guidance: as in `caption_batch`, one negative for every prompt or one each; a chunk then holds max_batch // 2
        prompts."""
        check_logprobs(logprobs)
        if attn_map is not None:
            AM.check_attn_map(attn_map, self.l["num_hidden_layers"])
        LR.check_logit_rules(logit_rules)
        prompts = [list(ids) for ids in list_of_input_ids]
        stops = None if stop is None else self._stop_records(stop, len(prompts), max_new_tokens)
        st = list(range(len(prompts))) if streams is None else [int(x) for x in streams]
        out: List[List[int]] = []
        gd = GD.check_guidance(guidance)
        if gd is not None:
            negs = self._negative_ids(gd, prompts)
            per = max(1, self.max_batch // 2)
            GD.pair_slots(1, self.max_batch)
            for c0 in range(0, len(prompts), per):
                chunk = prompts[c0:c0 + per]
                out += self.caption_batch([(pixels, ids) for ids in chunk], token_kept_ratio, max_new_tokens, eos_id, sampling=sampling,
                                          streams=st[c0:c0 + len(chunk)], share=[0] * len(chunk), logprobs=logprobs,
                                          logit_rules=logit_rules, attn_map=attn_map, stop=None if stops is None else stops[c0:c0 + len(chunk)],
                                          guidance=dict(scale=gd["scale"], negative_ids=negs[c0:c0 + len(chunk)]))
            return out
        for c0 in range(0, len(prompts), self.max_batch):
            chunk = prompts[c0:c0 + self.max_batch]
            out += self.caption_batch([(pixels, ids) for ids in chunk], token_kept_ratio, max_new_tokens, eos_id, sampling=sampling,
                                      streams=st[c0:c0 + len(chunk)], share=[0] * len(chunk),
                                      **({} if logprobs is None else dict(logprobs=logprobs)),
                                      **({} if logit_rules is None else dict(logit_rules=logit_rules)),
                                      **({} if attn_map is None else dict(attn_map=attn_map)),
                                      **({} if stops is None else dict(stop=stops[c0:c0 + len(chunk)])))
        return out

    # ------------------------------------------------------------------ continuous batching
    def slot_reset(self, slot: int):
        check(self.ctx, self.L.aur_slot_reset(self.ctx, slot, self._stream()), "aur_slot_reset")

    def slot_retire(self, slot: int):
        check(self.ctx, self.L.aur_slot_retire(self.ctx, slot, self._stream()), "aur_slot_retire")

    def slot_collect(self, slot0: int, nslots: int, ids_dev: torch.Tensor, lens_dev: torch.Tensor):
        """Async device copy of the ids / lengths of slots [slot0, slot0 + nslots) (no host synchronisation)."""
        assert ids_dev.dtype == torch.int32 and lens_dev.dtype == torch.int32 and ids_dev.is_contiguous() and lens_dev.is_contiguous()
        assert ids_dev.numel() >= nslots * self._max_new and lens_dev.numel() >= nslots
        check(self.ctx, self.L.aur_slot_collect(self.ctx, slot0, nslots, ids_dev.data_ptr(), lens_dev.data_ptr(), self._stream()),
              "aur_slot_collect")

    def slot_state(self):
        lens = np.zeros(self._batch, np.int32)
        fin = np.zeros(self._batch, np.int32)
        check(self.ctx, self.L.aur_slot_state(self.ctx, lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                              fin.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()), "aur_slot_state")
        return lens, fin

    def caption_stream(self, clips, token_kept_ratio: float, max_new_tokens: int, eos_id: Optional[int] = 2, slots: Optional[int] = None,
                       check_every: int = 16, on_error=None, overlap: Optional[bool] = None, front_cus: int = 16, front_graph: bool = True,
                       sampling: Optional[dict] = None, stream_of=None, share_key=None, logprobs: Optional[int] = None,
                       logit_rules: Optional[dict] = None, stop=None, attn_map: Optional[dict] = None, guidance: Optional[dict] = None):
        """Continuous batching over an iterable of (pixel_values, input_ids): up to `slots` (default max_batch) captions are
        in flight; every `check_every` decode steps the finished slots are collected and re-filled with the next clips
        (ViT + projector + prefill into the free slot while the others keep their KV and state).  Yields (index, ids) in
        completion order; each clip's ids equal what it produces alone (batch-invariant kernels).
        on_error(index, exception): a clip whose front end is rejected (shape, context longer than max_ctx, ...) is reported
        and skipped while the captions in flight keep going (the reference harness turns a failing request into an empty
        caption, lmms_eval/models/auroracap.py:511-514); None = raise.
        overlap (default: on when the engine was built with spare_slots > 0; whoever builds the engine decides with
        `streams.overlap_pays` whether a decode of that many slots is K / V-bound enough for it): the front ends of the NEXT clips run ahead on
        their own stream, restricted to `front_cus` CUs of every XCD, into the spare KV sequences while every slot keeps
        decoding (decode is HBM-bound, ViT + prefill MFMA-bound); a freed slot takes over a prepared clip's pages at the next
        check (`prefill_commit`).  front_graph (overlapped mode): each clip's front end is one hipGraph replay, captured per shape
        bucket on first use (`_front_end_replay`); False = ~600 eager launches per clip.  Same ids either way.
        sampling=dict(temperature, top_k, top_p, seed): sampled captions; a clip's stream is its index in `clips` (or
        stream_of(index), called when the clip is about to get its slot), whatever slot it lands in and whenever (a re-filled slot
        gets the new clip's record before its first token is picked).
        share_key: callable index -> hashable key | None (an engine built with prefix_cache >= 1).  Clips of equal key are the same
        visual input.  A keyed clip that misses the cache runs its normal front end, after which its leading whole pages are copied
        into a holder sequence (kept visual rows and plan beside it); one that hits runs no ViT: copy from the holder, its own plan
        spliced over the kept visual rows, and a prefill of the rows behind the fork only (`share_fork`; a clip that cannot fork takes
        the normal path).  In the overlapped mode such a front end runs eagerly on the front-end stream (never from a captured graph).
        Same ids either way.  An engine whose only spare sequences are holders must be called with overlap=False: the default
        follows spare_slots.
        logprobs=n: yields (index, dict) - ids, token_logprobs, top_ids, top_logprobs as in `generate` - in both modes, for clips
        from either front end.
        logit_rules: one dict for every clip of the call, as in `generate`; a re-filled slot gets its record where it gets its
        sampling record, before its first token is picked, and its history starts empty.
        stop: one dict for every clip of the call, as in `generate`, or a callable index -> dict | None, called where `stream_of` is
        (in the overlapped mode: when the clip's front end is prepared, so that a rejected record is the clip's own error).  A
        request's own max_new_tokens frees its slot at the next check after it is reached.  A re-filled slot gets its record where
        it gets its sampling and logit-rule records, in both modes and for sibling front ends too.  A callable counts as asking: the
        option is flipped when the call starts, since front-end graphs cannot be dropped while clips are staged behind them.
        attn_map: as in `generate` - yields (index, dict) with the clip's attn_map, the rows of a caption run alone, in both modes; a
        re-filled slot's rows are cleared where its length is.  keys=None: the engine's whole context rounded up to 64 (the prompts of
        a stream differ).
        guidance: not in this call yet - a pair of slots would have to travel through the staged commit and the row exchange
        together; a request (a scale other than None / 1) raises NotImplementedError."""
        if GD.check_guidance(guidance) is not None:
            raise NotImplementedError("caption_stream(guidance=...): guided requests go through generate / caption_ids / caption_batch / caption_prompts")
        lpn = check_logprobs(logprobs)
        samp = S.check_sampling(sampling)
        rules = LR.check_logit_rules(logit_rules)
        stop_of = None
        if callable(stop):
            stop_of = lambda idx: ST.check_stop(stop(idx), max_new_tokens, self._stop_table)      # noqa: E731
        elif stop is not None:
            one = ST.check_stop(stop, max_new_tokens, self._stop_table)
            stop_of = None if one is None else (lambda idx: one)
        if samp is not None:
            self._sampling_on()
        if rules is not None:
            self._rules_on()
        if stop_of is not None:
            self._stop_on()
        if lpn is not None:
            self._logprobs_on(lpn)
        amw = None if attn_map is None else self._attn_map_request(attn_map, None)
        B = self.max_batch if slots is None else slots
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"slots={B} for an engine built with max_batch={self.max_batch}")
        if share_key is not None and self.prefix_cache < 1:
            raise ValueError("caption_stream(share_key=) needs an engine built with prefix_cache >= 1")
        if overlap is None:
            overlap = self.spare_slots > 0
        n_hold = self.prefix_cache if share_key is not None else 0
        holders = _PrefixHolders(range(self.max_batch + self.spare_slots - n_hold, self.max_batch + self.spare_slots)) if n_hold else None
        if overlap:
            if self.spare_slots - n_hold < 1:
                raise ValueError("caption_stream(overlap=True) needs an engine built with spare_slots >= 1 beyond its prefix_cache")
            yield from self._caption_stream_overlapped(clips, token_kept_ratio, max_new_tokens, eos_id, B, check_every, on_error, front_cus,
                                                       front_graph, samp, stream_of, share_key, holders, lpn, rules, stop_of, amw)
            return
        self.begin_batch(B, max_new_tokens, eos_id)
        for s in range(B):
            self.slot_retire(s)
        it = iter(enumerate(clips))
        owner: List[Optional[int]] = [None] * B
        exhausted = False
        while True:
            for s in range(B):                                    # fill every free slot
                while owner[s] is None and not exhausted:
                    nxt = next(it, None)
                    if nxt is None:
                        exhausted = True
                        break
                    idx, (px, ids) = nxt
                    try:
                        r = self.tome_r(token_kept_ratio, px.shape[-2], px.shape[-1])
                        key = share_key(idx) if share_key is not None else None
                        hit = self._holder_hit(holders, key, px, list(ids), r) if key is not None else None
                        srec = ST.records([stop_of(idx)]) if stop_of is not None else None      # validated before anything is enqueued
                        if hit is not None:                       # a sibling: pages from the holder, then the rows behind the fork
                            h, fork, buf, stride, new = hit
                            self.kv_copy_prefix(h["seq"], s, 1, fork)
                            self.slot_reset(s)
                            if samp is not None:
                                self.slot_sampling(s, S.records(samp, [idx if stream_of is None else stream_of(idx)]))
                            if rules is not None:
                                self.slot_logit_rules(s, LR.records(rules, 1))
                            if srec is not None:
                                self.slot_stop(s, srec)
                            self.extend_batch(s, 1, buf, fork, stride, new)
                            owner[s] = idx
                            continue
                        vis = self.vit_encode(px, r)
                        plan = self.splice_plan(list(ids), vis.shape[0], vis.shape[1]) if key is not None else None
                        emb, L = self.project_splice(vis, list(ids), plan=plan)
                        self.slot_reset(s)
                        if samp is not None:
                            self.slot_sampling(s, S.records(samp, [idx if stream_of is None else stream_of(idx)]))
                        if rules is not None:
                            self.slot_logit_rules(s, LR.records(rules, 1))
                        if srec is not None:
                            self.slot_stop(s, srec)
                        self.prefill(s, emb, L)                   # argument checks come before any enqueue: a rejection leaves the slot idle
                        if key is not None:
                            self._holder_fill(holders, key, s, vis, plan, px, r)
                        owner[s] = idx
                    except (ValueError, IndexError, AssertionError, _lib.AuroraHipError) as e:
                        if on_error is None:
                            raise
                        on_error(idx, e)
            if all(o is None for o in owner):
                return
            self.decode(check_every)
            lens, fin = self.slot_state()
            done = [s for s in range(B) if owner[s] is not None and fin[s]]
            if done:
                out = (self.outputs(lpn) if amw is None else self._outputs(lpn, amw))
                for s in done:
                    yield owner[s], out[s]
                    owner[s] = None

    def _holder_hit(self, holders: "_PrefixHolders", key, px: torch.Tensor, ids: List[int], r: int):
        """A keyed clip against the holder cache: None (miss, another input shape, or a prompt that cannot fork) or (entry, fork, the
        rows [fork, seq_len) of its spliced prompt in a buffer of `stride` rows, stride, their number as the device tensor the extend
        calls read).  Everything the host can reject is rejected here, before anything touches a KV sequence."""
        e = holders.get(key)
        if e is None or e["shape"] != tuple(px.shape) or e["r"] != r:
            return None
        vis = e["vis"]
        host = splice_rows(ids, vis.shape[0], vis.shape[1])       # the decision needs no device: a prompt that cannot fork costs no upload
        fork = min(share_fork(e["plan"], host), e["tokens"])
        if fork <= 0:
            return None
        new = host["seq_len"] - fork
        stride = _rup(new, 32)
        check_seq_lens([new], stride, self._max_new, self.c.max_ctx, fork)
        # the device arrays of a prompt (three row maps and the length: blocking uploads) are built once per distinct prompt of the
        # call - a benchmark asks the same few questions about every video - and reused by every later hit
        pk = (tuple(ids), vis.shape[0], vis.shape[1], fork)
        if pk not in holders.plans:
            holders.plans[pk] = (self.splice_plan(ids, vis.shape[0], vis.shape[1]), torch.tensor([new], dtype=torch.int32, device=self.dev))
        plan, new_dev = holders.plans[pk]
        buf = torch.empty(stride, self.l["hidden_size"], dtype=torch.float16, device=self.dev)
        self._extend_rows(vis, plan, fork, buf)
        return e, fork, buf, stride, new_dev

    def _holder_fill(self, holders: "_PrefixHolders", key, seq: int, vis: torch.Tensor, plan: dict, px: torch.Tensor, r: int):
        """After the front end of a keyed clip that missed, on the stream that ran it: its leading whole pages go from KV sequence
        `seq` into a holder, its kept visual rows and plan are kept beside it.  A key that already has a holder keeps it (the clip
        could not fork from it: its prompt differs early), and so does a prompt shorter than a page."""
        tokens = fork_point(plan["seq_len"])
        if tokens <= 0 or plan["nvis"] < 1 or holders.get(key) is not None:
            return
        e = holders.put(key, vis=vis, plan=plan, shape=tuple(px.shape), r=r, tokens=tokens)
        if e is not None:
            self.kv_copy_prefix(seq, e["seq"], 1, tokens)

    def _masked_streams(self, front_cus: int):
        """(front-end stream on `front_cus` CUs of every XCD, decode stream on the other CUs); shared per process (streams.py)."""
        from .streams import shared_cu_masked_stream
        if not hasattr(self, "_masked"):
            self._masked = {}
        if front_cus not in self._masked:
            self._masked[front_cus] = (shared_cu_masked_stream(front_cus, device=self.dev),
                                       shared_cu_masked_stream(32 - front_cus, from_top=True, device=self.dev))
        return self._masked[front_cus]

    def _front_end_replay(self, px: torch.Tensor, ids: List[int], r: int, seq: int, front_cus: int):
        """ViT + ToMe + projector / splice + staged prefill of ONE clip into KV sequence `seq` as a single hipGraph replay on torch's
        current stream.  Graphs are captured per bank (its page table is baked in), per `front_cus` (so is the persistent GEMM's grid)
        and per shape bucket - (frames, H, W, r, prompt structure, seq) - on first use and kept (at most `front_graph_cap`, least
        recently used evicted): the per-bucket capture of the reference tree's serving engine
        (src/sglang/python/sglang/srt/model_executor/cuda_graph_runner.py:163-279).  Returns (embeds, seq_len) for `prefill_commit`
        - with `prompt_bucket`, (embeds, (stride, lengths buffer)): the bucket no longer depends on the exact prompt length -;
        `embeds` is the bucket's static buffer: the caller orders the next replay of the same bucket (same `seq`) after that commit.
        Third value: the graph that ran (its `vis` holds the clip's kept visual rows until the bucket's next replay)."""
        if px.dim() != 4 or px.shape[1] != self.v.get("num_channels", 3):
            raise ValueError(f"pixel_values must be [frames, {self.v.get('num_channels', 3)}, H, W], got {tuple(px.shape)}")
        F, H, W = int(px.shape[0]), int(px.shape[-2]), int(px.shape[-1])
        t0 = (H // self.v["patch_size"]) * (W // self.v["patch_size"]) + 1
        if F < 1 or F > self.c.max_frames or t0 < 2 or t0 > (self.max_image // self.v["patch_size"]) ** 2 + 1:
            raise ValueError(f"clip of {F} frames of {H}x{W} outside this engine (max_frames {self.c.max_frames}, max_image {self.max_image})")
        n_kept = tokens_at_layer(t0, r, self.v["num_hidden_layers"] - 1) - 1
        plan = self.splice_plan(ids, F, n_kept)
        if plan["seq_len"] < 1 or plan["seq_len"] + self._max_new > self.c.max_ctx:
            raise ValueError(f"prompt of {plan['seq_len']} positions + {self._max_new} new tokens exceeds max_ctx {self.c.max_ctx}")
        pb = self.prompt_bucket
        key = front_end_bucket_key(self._bank, front_cus, F, H, W, r, seq, plan, pb)
        if pb:
            stride, ntext_cap = key[7], key[10]
            if stride > _rup(self.c.max_ctx, self.c.page_tokens):
                raise ValueError(f"stride {stride} of prompt bucket {pb} exceeds the KV pages of a sequence (max_ctx {self.c.max_ctx})")
        cache = self._front_graphs
        fg = cache.pop(key, None)
        if fg is None:
            while len(cache) >= self.front_graph_cap:             # evict the least recently used bucket once its last replay has run
                _, old = next(iter(cache.items()))
                cache.pop(next(iter(cache)))
                if old._last is not None:
                    old._last.synchronize()
                old.close()
            if pb:
                fg = FrontEndGraph(self, 1, F, H, W, r, self.splice_plan(ids, F, n_kept, ntext_cap=ntext_cap), seq0=seq, stride=stride)
            else:
                fg = FrontEndGraph(self, 1, F, H, W, r, plan, seq0=seq)
            fg._last = None
        cache[key] = fg                                           # most recently used last
        fg.load(self._h(px), [plan])
        fg.launch()
        fg._last = torch.cuda.Event()
        fg._last.record(torch.cuda.current_stream(self.dev))
        return fg.embeds, ((fg.stride, fg.lens) if pb else plan["seq_len"]), fg

    def _caption_stream_overlapped(self, clips, token_kept_ratio, max_new_tokens, eos_id, B, check_every, on_error, front_cus, front_graph=True,
                                   samp=None, stream_of=None, share_key=None, holders=None, lpn=None, rules=None, stop_of=None, amw=None):
        from collections import deque
        sD = torch.cuda.current_stream(self.dev)
        sF, sDm = self._masked_streams(front_cus)
        self.begin_batch(B, max_new_tokens, eos_id)
        for s in range(B):
            self.slot_retire(s)
        it = iter(enumerate(clips))
        owner: List[Optional[int]] = [None] * B
        n_hold = len(holders.free) if holders is not None else 0                       # the last spare sequences hold shared prefixes
        free_seqs = list(range(self.max_batch, self.max_batch + self.spare_slots - n_hold))     # spare KV sequences holding no prepared clip
        reusable = {}                                             # sequence -> event after which its (exchanged) pages may be rewritten
        staged = deque()                                          # prepared clips: (index, sequence, embeds, L, event, stop record)
        exhausted = False
        sF.wait_stream(sD)
        self.set_option("gemm_max_wgs", 8 * front_cus)            # the persistent GEMM sizes its grid to the front end's CUs
        k_masked = max(1, int(round(0.8 * check_every)))
        try:
            while True:
                # 1. slots that are free take over prepared clips (decode stream, between two decode calls)
                for s in range(B):
                    if owner[s] is None and staged:
                        idx, seq, emb, L, ev, srec = staged.popleft()
                        sD.wait_event(ev)
                        emb.record_stream(sD)
                        if samp is not None:                      # the captured front end holds the stage only: the pick is the commit's
                            self.slot_sampling(s, S.records(samp, [idx if stream_of is None else stream_of(idx)]))
                        if rules is not None:                     # begin_batch made every slot neutral; a commit keeps a slot's record
                            self.slot_logit_rules(s, LR.records(rules, 1))
                        if srec is not None:                      # a neutral record too: the commit keeps what the slot's last clip left
                            self.slot_stop(s, srec)
                        if isinstance(L, tuple) and L[0] == "extend":     # a sibling staged behind a copied prefix: (_, fork, stride, rows)
                            L[3].record_stream(sD)
                            self.extend_commit(s, 1, seq, emb, L[1], L[2], L[3])
                        elif isinstance(L, tuple):                # a bucketed front end: (stride, the graph's static lengths buffer)
                            self.prefill_commit(s, 1, seq, emb, L[0], seq_lens=L[1])
                        else:
                            self.prefill_commit(s, 1, seq, emb, L)
                        evc = torch.cuda.Event()
                        evc.record(sD)
                        reusable[seq] = evc
                        free_seqs.append(seq)
                        owner[s] = idx
                # 2. one decode chunk, enqueued BEFORE the next front ends (a few hundred launches on the host: the decode must not
                #    sit behind them); while a front end will be in flight its first part runs on the complementary CU mask
                decoding = any(o is not None for o in owner)
                if decoding:
                    k1 = min(check_every, k_masked) if (free_seqs and not exhausted) else 0
                    if k1 > 0:
                        sDm.wait_stream(sD)
                        with torch.cuda.stream(sDm):
                            # on half of the CUs the QKV / gate-up projections launch half as many workgroups with twice the tiles each
                            # (bitwise the same tokens; engines of <= 64 slots ignore it)
                            self.set_option("decode_half_grid", 1)
                            try:
                                self.decode(k1)
                            finally:                                # a failed decode must not leave the ctx replaying the half-grid graph
                                self.set_option("decode_half_grid", 0)
                        sD.wait_stream(sDm)
                    if check_every - k1 > 0:
                        self.decode(check_every - k1)
                # 3. prepare the next clips into every free spare sequence (front-end stream: runs beside the decode above)
                while free_seqs and not exhausted:
                    # the iterator may be lazy (the lmms-eval adaptor decodes and preprocesses a clip when asked): whatever it
                    # enqueues on torch's current stream must be ordered before the front end that reads it -> pull the clip
                    # with the front-end stream current, so its kernels and allocations belong to that stream
                    with torch.cuda.stream(sF):
                        nxt = next(it, None)
                    if nxt is None:
                        exhausted = True
                        break
                    idx, (px, ids) = nxt
                    seq = free_seqs.pop()
                    try:
                        with torch.cuda.stream(sF):
                            if torch.is_tensor(px) and px.is_cuda:
                                px.record_stream(sF)              # allocated on another stream (a prebuilt clip): not reusable before sF is done with it
                            if seq in reusable:
                                sF.wait_event(reusable.pop(seq))
                            r = self.tome_r(token_kept_ratio, px.shape[-2], px.shape[-1])
                            srec = ST.records([stop_of(idx)]) if stop_of is not None else None
                            key = share_key(idx) if share_key is not None else None
                            hit = self._holder_hit(holders, key, px, list(ids), r) if key is not None else None
                            if hit is not None:                   # a sibling: no ViT, eager on this stream into its spare sequence
                                h, fork, emb, stride, new = hit
                                self.kv_copy_prefix(h["seq"], seq, 1, fork)
                                self.extend_stage(seq, 1, emb, fork, stride, new)
                                L = ("extend", fork, stride, new)
                            elif front_graph:
                                emb, L, fg = self._front_end_replay(px, list(ids), r, seq, front_cus)  # one hipGraph replay per clip (captured per bucket)
                                if key is not None:
                                    # the graph's visual rows are a static buffer: the holder keeps a copy.  Its plan is the host form
                                    # (`splice_rows`): a holder's plan is only ever compared (`share_fork`), a sibling is spliced with its own
                                    self._holder_fill(holders, key, seq, fg.vis[:px.shape[0]].clone(), splice_rows(list(ids), px.shape[0], fg.n_kept),
                                                      px, r)
                            else:
                                vis = self.vit_encode(px, r)
                                plan = self.splice_plan(list(ids), vis.shape[0], vis.shape[1]) if key is not None else None
                                emb, L = self.project_splice(vis, list(ids), plan=plan)
                                self.prefill_stage(seq, 1, emb, L)    # argument checks come before any enqueue
                                if key is not None:               # before the event the commit waits on: the exchange comes later
                                    self._holder_fill(holders, key, seq, vis, plan, px, r)
                            ev = torch.cuda.Event()
                            ev.record(sF)
                        staged.append((idx, seq, emb, L, ev, srec))
                    except (ValueError, IndexError, AssertionError, _lib.AuroraHipError) as e:
                        free_seqs.append(seq)
                        if on_error is None:
                            raise
                        on_error(idx, e)
                if not decoding:
                    if not staged:
                        return
                    continue                                      # nothing decoding yet: commit what was just prepared
                lens, fin = self.slot_state()
                done = [s for s in range(B) if owner[s] is not None and fin[s]]
                if done:
                    out = (self.outputs(lpn) if amw is None else self._outputs(lpn, amw))
                    for s in done:
                        yield owner[s], out[s]
                        owner[s] = None
        finally:
            sD.wait_stream(sF)
            self.set_option("gemm_max_wgs", 0)

    # ------------------------------------------------------------------ captured call sequences (hipGraph)
    def graph_capture(self, fn):
        """Record the engine calls `fn()` enqueues on torch's current stream into a hipGraph (aur_graph_begin / aur_graph_end) and
        return (handle, number of nodes).  `fn` must only make enqueue-only engine calls on pre-allocated tensors: a torch
        allocation, a synchronisation or `decode` inside it breaks the capture (raised here)."""
        st = self._stream()
        check(self.ctx, self.L.aur_graph_begin(self.ctx, st), "aur_graph_begin")
        gid, nodes = C.c_int32(0), C.c_int64(0)
        try:
            fn()
        except BaseException:
            self.L.aur_graph_end(self.ctx, st, C.byref(gid), C.byref(nodes))      # always close the capture; its status is secondary
            if gid.value:
                self.L.aur_graph_destroy(self.ctx, gid.value)
            raise
        check(self.ctx, self.L.aur_graph_end(self.ctx, st, C.byref(gid), C.byref(nodes)), "aur_graph_end")
        return gid.value, nodes.value

    def graph_launch(self, gid: int):
        check(self.ctx, self.L.aur_graph_launch(self.ctx, gid, self._stream()), "aur_graph_launch")

    def graph_destroy(self, gid: int):
        check(self.ctx, self.L.aur_graph_destroy(self.ctx, gid), "aur_graph_destroy")

    def decode_stamps(self, cap: int = 4096):
        """(microseconds per step of the stamped attention launch, oldest first; total steps stamped) - option
        "decode_stamp_layer"; synchronises."""
        buf = (C.c_double * cap)()
        n, tot = C.c_int32(0), C.c_int64(0)
        check(self.ctx, self.L.aur_decode_stamps_read(self.ctx, buf, cap, C.byref(tot), C.byref(n), self._stream()), "aur_decode_stamps_read")
        return np.asarray(buf[:n.value], dtype=np.float64), tot.value

    # ------------------------------------------------------------------ kernel-level entry points (tests)
    def tome_step(self, metric: torch.Tensor, x: torch.Tensor, size: Optional[torch.Tensor], r: int):
        F, t, c = metric.shape
        d = x.shape[-1]
        rl = max(0, min(r, (t - 1) // 2))
        ta = (t + 1) // 2
        m = self._f(metric)
        xh = self._h(x)
        s = self._f(size.reshape(F, t)) if size is not None else None
        xo = torch.empty(F, t - rl, d, dtype=torch.float16, device=self.dev)
        so = torch.empty(F, t - rl, dtype=torch.float32, device=self.dev)
        ni = torch.zeros(F, ta, dtype=torch.int32, device=self.dev)
        un = torch.zeros(F, max(ta - rl, 1), dtype=torch.int32, device=self.dev)
        sr = torch.zeros(F, max(rl, 1), dtype=torch.int32, device=self.dev)
        ds = torch.zeros(F, max(rl, 1), dtype=torch.int32, device=self.dev)
        check(self.ctx, self.L.aur_tome_step(self.ctx, m.data_ptr(), xh.data_ptr(), s.data_ptr() if s is not None else None,
                                             F, t, c, d, r, xo.data_ptr(), so.data_ptr(), ni.data_ptr(), un.data_ptr(),
                                             sr.data_ptr(), ds.data_ptr(), self._stream()), "aur_tome_step")
        torch.cuda.synchronize()
        return xo, so, dict(r=rl, node_idx=ni, unm_idx=un[:, : ta - rl], src_idx=sr[:, :rl], dst_idx=ds[:, :rl])

    def tome_map_rows(self, rows: torch.Tensor, t: int, r: int, unm: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        """One step of the merge map on caller data, in place (`merge_map.step_rows`; aur_tome_map_rows): rows int32 [F, n] on the
        device, every entry the row of a step over `t` rows; unm [F, ceil(t/2) - r], src / dst [F, r] as `tome_step` returns them;
        r already clamped to (t - 1) // 2.  Returns `rows`."""
        if not (torch.is_tensor(rows) and rows.dim() == 2 and rows.dtype == torch.int32 and rows.is_contiguous() and rows.is_cuda):
            raise ValueError("rows must be a contiguous int32 [frames, n] tensor on the device (it is rewritten in place)")
        F, n = rows.shape
        t, r = int(t), int(r)
        if F < 1 or n < 1 or t < 1 or t > 8192:
            raise ValueError(f"frames {F}, n {n}, t {t}: all >= 1 and t <= 8192")
        if r < 0 or r > (t - 1) // 2:
            raise ValueError(f"r = {r} outside [0, (t - 1) // 2 = {(t - 1) // 2}]")
        idx = []
        for name, a, w in (("unm", unm, (t + 1) // 2 - r), ("src", src, r), ("dst", dst, r)):
            if r == 0:
                idx.append(None)
                continue
            if not torch.is_tensor(a) or a.numel() != F * w:
                raise ValueError(f"{name} must hold [frames, {w}] = {F * w} indices")
            idx.append(a.to(device=self.dev, dtype=torch.int32).contiguous())
        ptr = [a.data_ptr() if a is not None else None for a in idx]
        check(self.ctx, self.L.aur_tome_map_rows(self.ctx, rows.data_ptr(), F, n, t, r, ptr[0], ptr[1], ptr[2], self._stream()),
              "aur_tome_map_rows")
        return rows

    def unmerge(self, tokens: torch.Tensor, map: torch.Tensor) -> torch.Tensor:
        """tokens [F, n_kept, d], map int [F, ...] -> fp16 [F, ..., d]: every patch gets the row of the token it was merged into
        (`merge_map.unmerge`; aur_unmerge_rows).  d a multiple of 8."""
        if not torch.is_tensor(tokens) or tokens.dim() != 3:
            raise ValueError("tokens must be [frames, n_kept, d]")
        if not torch.is_tensor(map) or map.dim() < 2 or map.shape[0] != tokens.shape[0] or map.is_floating_point():
            raise ValueError(f"map must be an integer [frames = {tokens.shape[0]}, ...] tensor")
        F, n_kept, d = tokens.shape
        if d % 8:
            raise ValueError(f"d = {d} is not a multiple of 8")
        n = map[0].numel()
        if F < 1 or n < 1 or n_kept < 1:
            raise ValueError("empty tokens or map")
        tk = self._h(tokens)
        mp = map.to(device=self.dev, dtype=torch.int32).contiguous()
        out = torch.empty(*map.shape, d, dtype=torch.float16, device=self.dev)
        check(self.ctx, self.L.aur_unmerge_rows(self.ctx, tk.data_ptr(), mp.data_ptr(), F, n, n_kept, d, out.data_ptr(), self._stream()),
              "aur_unmerge_rows")
        return out

    def linear(self, a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = 0,
               resid: Optional[torch.Tensor] = None) -> torch.Tensor:
        n, k = w.shape
        npad = _rup(n, 256)
        wp = self.pack(w, npad, k)
        b = self._bias(bias, npad) if bias is not None else None
        ah = self._h(a)
        rh = self._h(resid) if resid is not None else None
        out = torch.empty(ah.shape[0], n, dtype=torch.float16, device=self.dev)
        check(self.ctx, self.L.aur_linear(self.ctx, ah.data_ptr(), ah.shape[0], k, wp.data_ptr(), npad, n,
                                          b.data_ptr() if b is not None else None, act, rh.data_ptr() if rh is not None else None,
                                          out.data_ptr(), self._stream()), "aur_linear")
        torch.cuda.synchronize()
        return out

    def gemm_rows(self, a: torch.Tensor, w_packed: torch.Tensor, n: int, c: torch.Tensor, *, m: Optional[int] = None, k: Optional[int] = None,
                  ldc: Optional[int] = None, bias: Optional[torch.Tensor] = None, act: int = 0, tag: int = 0, resid: Optional[torch.Tensor] = None,
                  in_place: bool = False, out_rows=None) -> torch.Tensor:
        """aur_gemm_rows: one EPI_ROW tile-GEMM launch on caller buffers.  a fp16 [rows, lda]: the operand is its first `m` rows (default
        all; later rows are the caller's guard) by its first `k` columns (default all).  w_packed [npad, k] from `pack`; bias fp32 [npad].
        `c` is the INITIAL content of the output - sentinels outside the stored set survive - with rows `ldc` halves apart (default: its
        width; a flat tensor carries a guard behind the last row).  resid fp16 [rows >= m, ldr], or in_place: read from c itself.
        out_rows: int32 [m], list or device tensor.  Returns the device copy of c as it is after the launch."""
        ah = self._h(a)
        m = ah.shape[0] if m is None else m
        lda = ah.shape[1]
        k = lda if k is None else k
        npad = w_packed.numel() // k
        ldc = c.shape[-1] if ldc is None else ldc
        o = self._h(c).clone()
        rh = self._h(resid) if resid is not None else None
        rows_t = self._i32_arg(out_rows, m, "out_rows") if out_rows is not None else None
        b = self._f(bias) if bias is not None else None
        if b is not None and b.numel() < npad:
            raise ValueError(f"bias of {b.numel()} entries for npad {npad}")
        ptr = lambda t: t.data_ptr() if t is not None else None
        check(self.ctx, self.L.aur_gemm_rows(self.ctx, ah.data_ptr(), m, k, lda, w_packed.data_ptr(), npad, n, ptr(b), act, tag,
                                             o.data_ptr() if in_place else ptr(rh), ldc if in_place else (rh.shape[1] if rh is not None else 0),
                                             ptr(rows_t), o.data_ptr(), ldc, self._stream()), "aur_gemm_rows")
        torch.cuda.synchronize()
        return o

    def linear_skinny(self, a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        n, k = w.shape
        npad = _rup(n, 256)
        wp = self.pack(w, npad, k)
        ah = self._h(a)
        out = torch.empty(ah.shape[0], n, dtype=torch.float32, device=self.dev)
        check(self.ctx, self.L.aur_linear_skinny(self.ctx, ah.data_ptr(), ah.shape[0], k, wp.data_ptr(), npad, n, out.data_ptr(),
                                                 self._stream()), "aur_linear_skinny")
        torch.cuda.synchronize()
        return out

    def layernorm(self, x, w, b, eps):
        xh = self._h(x)
        y = torch.empty_like(xh)
        wf, bf = self._f(w), self._f(b)
        check(self.ctx, self.L.aur_layernorm(self.ctx, xh.data_ptr(), xh.shape[0], xh.shape[1], wf.data_ptr(), bf.data_ptr(),
                                             eps, y.data_ptr(), self._stream()), "aur_layernorm")
        torch.cuda.synchronize()
        return y

    def rmsnorm(self, x, w, eps):
        xh = self._h(x)
        y = torch.empty_like(xh)
        wf = self._f(w)
        check(self.ctx, self.L.aur_rmsnorm(self.ctx, xh.data_ptr(), xh.shape[0], xh.shape[1], wf.data_ptr(), eps, y.data_ptr(),
                                           self._stream()), "aur_rmsnorm")
        torch.cuda.synchronize()
        return y

    def vit_layer(self, layer: int, x: torch.Tensor, size: Optional[torch.Tensor], r: int):
        F, t, D = x.shape
        hd = D // self.v["num_attention_heads"]
        rl = max(0, min(r, (t - 1) // 2))
        ta = (t + 1) // 2
        xh = self._h(x)
        s = self._f(size.reshape(F, t)) if size is not None else None
        xo = torch.empty(F, t - rl, D, dtype=torch.float16, device=self.dev)
        so = torch.empty(F, t - rl, dtype=torch.float32, device=self.dev)
        me = torch.zeros(F, t, hd, dtype=torch.float32, device=self.dev)
        ni = torch.zeros(F, ta, dtype=torch.int32, device=self.dev)
        un = torch.zeros(F, max(ta - rl, 1), dtype=torch.int32, device=self.dev)
        sr = torch.zeros(F, max(rl, 1), dtype=torch.int32, device=self.dev)
        ds = torch.zeros(F, max(rl, 1), dtype=torch.int32, device=self.dev)
        check(self.ctx, self.L.aur_vit_layer(self.ctx, layer, xh.data_ptr(), s.data_ptr() if s is not None else None, F, t, r,
                                             xo.data_ptr(), so.data_ptr(), me.data_ptr(), ni.data_ptr(), un.data_ptr(),
                                             sr.data_ptr(), ds.data_ptr(), self._stream()), "aur_vit_layer")
        torch.cuda.synchronize()
        return xo, so, me, dict(r=rl, node_idx=ni, unm_idx=un[:, : ta - rl], src_idx=sr[:, :rl], dst_idx=ds[:, :rl])

    def attn_identity_weight(self, layout: str) -> torch.Tensor:
        """the identity [3 D, 3 D] packed with the loader's QKV row map of `layout` ("vit" / "llm"): with x = [q | k | v] the QKV
        epilogue then writes exactly the caller's q, k, v into the attention's fragments"""
        m = self.v if layout == "vit" else self.l
        D, H = m["hidden_size"], m["num_attention_heads"]
        if layout == "vit":
            npad = _rup(2 * _rup(H * _rup(D // H, 32), 64) + D, 256)
            rm = self.vit_qkv_row_map(D, H, npad)
        else:
            npad = _rup(3 * D, 256)
            rm = self.llama_qkv_row_map(D, H, npad)
        return self.pack(torch.eye(3 * D), npad, 3 * D, rm)

    def attn_rows(self, x: torch.Tensor, w_packed: torch.Tensor, *, layout: str, nseq: int, rows: int, causal: bool, t: Optional[int] = None,
                  lens=None, rope: bool = False, seq0: int = 0, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """aur_attn_rows: the QKV epilogue + attn_kernel on caller rows x [nseq * rows, kx]; `t` valid keys / queries by value, or `lens`
        (one per sequence) through device memory.  Returns fp16 [nseq * rows, heads * head_dim]."""
        m = self.v if layout == "vit" else self.l
        xh = self._h(x)
        kx = xh.shape[1]
        assert xh.shape[0] == nseq * rows and (t is None) != (lens is None)
        lens_t = self._i32_arg(lens, nseq, "lens") if lens is not None else None
        out = torch.empty(nseq * rows, m["hidden_size"], dtype=torch.float16, device=self.dev)
        check(self.ctx, self.L.aur_attn_rows(self.ctx, 0 if layout == "vit" else 1, xh.data_ptr(), nseq, rows, kx, w_packed.data_ptr(),
                                             w_packed.numel() // kx, bias.data_ptr() if bias is not None else None, seq0, int(rope),
                                             int(t or 0), lens_t.data_ptr() if lens_t is not None else None, int(causal), out.data_ptr(),
                                             self._stream()), "aur_attn_rows")
        torch.cuda.synchronize()
        return out

    def attn_decode_rows(self, x: torch.Tensor, w_packed: torch.Tensor, pos, *, rope: bool = False) -> torch.Tensor:
        """aur_attn_decode_rows: one decode step's QKV write + decode attention on caller rows x [B, kx]; pos[b] = tokens already cached
        for KV sequence b.  Returns fp16 [B, hidden]."""
        xh = self._h(x)
        B, kx = xh.shape
        pos_t = self._i32_arg(pos, B, "pos")
        scratch = torch.empty(self.L.aur_attn_decode_scratch_bytes(self.ctx, kx), dtype=torch.uint8, device=self.dev)
        out = torch.empty(B, self.l["hidden_size"], dtype=torch.float16, device=self.dev)
        check(self.ctx, self.L.aur_attn_decode_rows(self.ctx, xh.data_ptr(), B, kx, w_packed.data_ptr(), w_packed.numel() // kx,
                                                    pos_t.data_ptr(), int(rope), scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                                    self._stream()), "aur_attn_decode_rows")
        torch.cuda.synchronize()
        return out

    PROJ_MODES = {"row": 0, "logits": 1, "silu_mul": 2}

    def decode_proj_rows(self, mode: str, x: torch.Tensor, w_packed: torch.Tensor, n: int, out: torch.Tensor, *, b0: int = 0, fold: bool = False,
                         eps: float = 1e-5, fill: float = 0.0, ssq_out: Optional[torch.Tensor] = None, ssq_in: Optional[torch.Tensor] = None) -> dict:
        """aur_decode_proj_rows: one decode projection ("row", "silu_mul", "logits") on caller rows x [rows, k] at batch rows [b0, b0 + rows).
        `out` is the initial content of the output for all round_up(max_batch, 16) batch rows: the residual fp16 [rp, n] ("row"), the
        sentinel fp16 [rp, n / 2] ("silu_mul"), or fp32 [rp * n + guard] ("logits").  ssq_out / ssq_in: initial int64 [16, 128] arrays.
        Returns dict(out, ssq_out, ssq_in, ssq_zero, row_cnt) of device tensors as they are after the launch (None where unused)."""
        xh = self._h(x)
        rows, k = xh.shape
        npad = w_packed.numel() // k
        o = out.detach().to(self.dev).contiguous().clone()
        zeros = lambda: torch.zeros(16, 128, dtype=torch.int64, device=self.dev)
        so = ssq_out.to(self.dev).contiguous().clone() if ssq_out is not None else (zeros() if mode == "row" else None)
        si = (ssq_in.to(self.dev).contiguous().clone() if ssq_in is not None else zeros()) if fold else None
        sz = zeros() if fold else None
        cnt = torch.full((npad // 16,), -1, dtype=torch.int32, device=self.dev) if mode == "row" else None
        scratch = torch.empty(self.L.aur_decode_proj_scratch_bytes(self.ctx, k, npad), dtype=torch.uint8, device=self.dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        check(self.ctx, self.L.aur_decode_proj_rows(self.ctx, self.PROJ_MODES[mode], xh.data_ptr(), rows, b0, k, w_packed.data_ptr(), npad, n,
                                                    int(fold), eps, fill, o.data_ptr(), o.numel() * o.element_size(), ptr(so), ptr(si), ptr(sz),
                                                    ptr(cnt), scratch.data_ptr(), scratch.numel(), self._stream()), "aur_decode_proj_rows")
        torch.cuda.synchronize()
        return dict(out=o, ssq_out=so, ssq_in=si, ssq_zero=sz, row_cnt=cnt)

    def set_option(self, name: str, value: int):
        check(self.ctx, self.L.aur_set_option(self.ctx, name.encode(), int(value)), "aur_set_option")

    def microbench(self, kernel: str, iters: int = 200) -> float:
        us = C.c_double(0)
        check(self.ctx, self.L.aur_microbench(self.ctx, kernel.encode(), iters, C.byref(us), self._stream()), "aur_microbench")
        return us.value

    # ------------------------------------------------------------------ profiling
    def profile(self, on: bool):
        check(self.ctx, self.L.aur_profile_enable(self.ctx, int(on)), "aur_profile_enable")

    def profile_read(self, stage: str):
        ms, n = C.c_double(0), C.c_int64(0)
        check(self.ctx, self.L.aur_profile_read(self.ctx, stage.encode(), C.byref(ms), C.byref(n)), "aur_profile_read")
        return ms.value, n.value


class FrontEndGraph:
    """The front end of a GROUP of `group` equal-shape clips - ViT + per-layer ToMe, projector + splice, and the staged prefill
    of the group into KV sequences [seq0, seq0 + group) - captured once into a hipGraph and replayed with one call.

    The reference tree's own serving engine captures one graph per shape bucket and copies each request's inputs into the graph's
    static buffers before the replay (src/sglang/python/sglang/srt/model_executor/cuda_graph_runner.py:163-279); the bucket here is
    (group, frames, H, W, r, prompt structure, seq0), the static buffers are `pixels`, the three splice-plan arrays and `embeds`.
    The graph writes through the page table of the bank current at construction: `launch` refuses to run in another bank.
    A front end is ~600 launches (31 ViT layers x 10 + 32 prefill layers x 8 + splices): replayed from the graph the host submits it
    in one call, so a serving loop can submit it just before the device can start it (bounded run-ahead: host-observed TTFT stays
    close to the device's) without starving the front-end stream.

        fg = FrontEndGraph(eng, group, frames, H, W, r, plan, seq0, embeds=emb)     # on the stream that will replay it
        fg.load(pixels, plans); fg.launch()                                        # per group; then eng.prefill_commit(.., fg.embeds, ..)
    """

    def __init__(self, eng: "AuroraCapEngine", group: int, frames: int, height: int, width: int, r: int, plan: dict, seq0: int,
                 embeds: Optional[torch.Tensor] = None, prefill: str = "stage", slot0: int = 0, stride: Optional[int] = None):
        v, d = eng.v, eng.l["hidden_size"]
        # stride: the variable-length form.  The sequences lie `stride` rows apart, `plan` is a padded one (`splice_plan(ntext_cap=)`,
        # its capacity becomes the bucket's) and the lengths are one more static buffer, `lens`, read by the captured kernels at replay:
        # the graph serves every prompt of this structure whose length fits the stride and whose text fits the capacity.
        self.stride = stride
        self.eng, self.group, self.frames, self.r, self.seq0 = eng, group, frames, r, seq0
        self.bank = eng._bank                                     # the graph writes through this bank's page table
        self.seq_len = plan["seq_len"]
        self.mseq = _rup(self.seq_len, 32) if stride is None else stride
        if stride is not None and (plan.get("ntext_cap") is None or self.seq_len > stride):
            raise ValueError("the variable-length front end needs a padded splice plan that fits the stride")
        t0 = (height // v["patch_size"]) * (width // v["patch_size"]) + 1
        self.n_kept = tokens_at_layer(t0, r, v["num_hidden_layers"] - 1) - 1
        assert not np.isscalar(plan["n_kept"]) or plan["n_kept"] == self.n_kept
        dev = eng.dev
        self.pixels = torch.zeros(group * frames, v.get("num_channels", 3), height, width, dtype=torch.float16, device=dev)
        self.vis = torch.empty(group * frames, self.n_kept, v["hidden_size"], dtype=torch.float16, device=dev)
        self.embeds = embeds if embeds is not None else torch.zeros(group * self.mseq, d, dtype=torch.float16, device=dev)
        assert self.embeds.shape[0] >= group * self.mseq and self.embeds.is_contiguous()
        # the bucket's splice plans: same structure as `plan` (row maps of one prompt), contents replaced per clip by load()
        self.used, self.nvis, self.ntext = plan["used"], plan["nvis"], plan["ntext"] if stride is None else plan["ntext_cap"]
        self.lens = torch.ones(group, dtype=torch.int32, device=dev)
        self.vis_rows = torch.zeros(group, max(self.nvis, 1), dtype=torch.int32, device=dev)
        self.text_ids = torch.zeros(group, max(self.ntext, 1), dtype=torch.int32, device=dev)
        self.text_rows = torch.zeros(group, max(self.ntext, 1), dtype=torch.int32, device=dev)
        self._plans = [dict(seq_len=self.seq_len, used=self.used, n_kept=plan["n_kept"], nvis=self.nvis, ntext=self.ntext,
                            vis_rows=self.vis_rows[j], text_ids=self.text_ids[j], text_rows=self.text_rows[j]) for j in range(group)]
        eng.interpolated_pos(height, width)                       # the position table of this input size exists before the capture
        for j in range(group):
            self.vis_rows[j].copy_(plan["vis_rows"])
            self.text_ids[j].copy_(plan["text_ids"])
            self.text_rows[j].copy_(plan["text_rows"])
            self.lens[j:j + 1].copy_(plan["len_dev"])

        def run():
            eng.vit_encode(self.pixels, r, out=self.vis)
            for j in range(group):
                eng.project_splice(self.vis[j * frames:(j + 1) * frames], plan=self._plans[j], out=self.embeds[j * self.mseq:(j + 1) * self.mseq],
                                   stride=stride)
            var = dict(seq_lens=self.lens) if stride is not None else {}
            if prefill == "stage":
                eng.prefill_stage(seq0, group, self.embeds, self.mseq if var else self.seq_len, **var)
            elif prefill == "batch":
                eng.prefill_batch(slot0, group, self.embeds, self.mseq if var else self.seq_len, **var)
            else:
                assert prefill == "none"

        run()                                                      # once eagerly: lazily set kernel attributes must not happen inside a capture
        self.gid, self.nodes = eng.graph_capture(run)

    def load(self, pixels: torch.Tensor, plans: Optional[Sequence[dict]] = None, *, vis_rows=None, text_ids=None, text_rows=None):
        """Copy a group's inputs into the graph's static buffers (device-to-device on torch's current stream).  plans: the clips'
        `splice_plan`s (same structure as the bucket's), or stacked [group, n] int32 arrays through the keyword arguments."""
        self.pixels.copy_(pixels.reshape(self.pixels.shape), non_blocking=True)
        if plans is not None:
            assert len(plans) == self.group
            for j, pl in enumerate(plans):
                if self.stride is not None:
                    if (pl["used"], pl["nvis"]) != (self.used, self.nvis) or pl["seq_len"] > self.stride or pl["ntext"] > self.ntext:
                        raise ValueError("splice plan of another shape bucket")
                    n = pl["ntext"]                               # the clip's own plan may be exact or padded: entries beyond n are unused
                    self.text_rows[j].fill_(-1)
                    self.vis_rows[j, :self.nvis].copy_(pl["vis_rows"], non_blocking=True)
                    self.text_ids[j, :n].copy_(pl["text_ids"][:n], non_blocking=True)
                    self.text_rows[j, :n].copy_(pl["text_rows"][:n], non_blocking=True)
                    self.lens[j:j + 1].copy_(pl["len_dev"], non_blocking=True)
                    continue
                if (pl["seq_len"], pl["used"], pl["nvis"], pl["ntext"]) != (self.seq_len, self.used, self.nvis, self.ntext):
                    raise ValueError("splice plan of another shape bucket")
                self.vis_rows[j, :self.nvis].copy_(pl["vis_rows"], non_blocking=True)
                self.text_ids[j, :self.ntext].copy_(pl["text_ids"], non_blocking=True)
                self.text_rows[j, :self.ntext].copy_(pl["text_rows"], non_blocking=True)
        if vis_rows is not None:
            self.vis_rows.copy_(vis_rows, non_blocking=True)
        if text_ids is not None:
            self.text_ids.copy_(text_ids, non_blocking=True)
        if text_rows is not None:
            self.text_rows.copy_(text_rows, non_blocking=True)

    def launch(self):
        if self.eng._bank != self.bank:
            raise ValueError(f"front end captured in bank {self.bank} launched in bank {self.eng._bank}")
        self.eng.graph_launch(self.gid)

    def close(self):
        if self.gid:
            self.eng.graph_destroy(self.gid)
            self.gid = 0

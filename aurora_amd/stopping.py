"""How a generation ends, as this package defines it, restated in numpy.  No GPU, no torch.

    reason = fires(h, record, table, eos, batch_max_new)

is what the device decides behind the pick of the newest token of `h`: `advance_tail` (EOS, a full output row) and `stop_check_kernel`
(everything else) together.  `h` is the ids a slot has GENERATED, the prompt never included, n = len(h) >= 1 and t = h[n - 1] the token
just appended.  A request's stop record has three parts:

  * token_ids: 0 to 8 ids;
  * strings: 0 to 8 strings, each 1 to 64 bytes of UTF-8;
  * max_new_tokens: 0 = the batch's limit, otherwise 1 up to the batch's limit.

`table` = (offsets int32 [V + 1], bytes uint8 [...]) holds the bytes every vocabulary entry decodes to (`token_bytes`): for a fast
tokenizer the text `convert_tokens_to_string` gives the token behind a fixed prefix, prefix removed, as UTF-8 - the trick of
transformers' `StopStringCriteria.clean_tokenizer_vocab` -; a byte-fallback token `<0xNN>` is the single byte NN.

The slot stops behind t if one of these holds; the first that does, in this order, is the reason:

  1. "eos": t is the batch's EOS (today's rule, decided in `advance_tail`);
  2. "stop_token": t is one of token_ids;
  3. "stop_string": in the concatenation of the bytes of h, some occurrence of one of `strings` overlaps the bytes of t - it ends inside
     t's bytes or at their end.  Overhang on both sides counts (["las", "topper"] stops on "stop"); an occurrence that ends before t
     begins does not (["stop", "at"] does not stop).  A token of zero bytes never completes a string.  An id outside the table
     contributes no bytes and breaks the text at that point.  The index reported is the lowest index of a string that matches;
  4. "length": n has reached the record's max_new_tokens or the batch's.

In every case t stays in the output, as the EOS does and as transformers does with a stop string.  Rule 3 is `StopStringCriteria`'s
verdict stated as text: on tests/golden/ckpt_tiny's tokenizer the two agree on every one of 3000 random sequences
(tests/test_stopping_host.py).  They can differ only through zero-byte tokens and ids outside the table, where the text rule above is
the definition.

`min_new_tokens` (aurora_amd.logit_rules) keeps banning the batch's EOS only: stop ids and stop strings are criteria, not logits, and
apply from the first generated token.
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_IDS, MAX_STRINGS, MAX_STRING_BYTES, MAX_TOKEN_BYTES = 8, 8, 64, 255
# aur_stop_rules (include/aurora_hip.h), field for field
RECORD = np.dtype([("max_new_tokens", "<i4"), ("n_token_ids", "<i4"), ("n_strings", "<i4"), ("reserved", "<i4"),
                   ("token_ids", "<i4", (MAX_IDS,)), ("string_len", "<i4", (MAX_STRINGS,)), ("strings", "u1", (MAX_STRINGS, MAX_STRING_BYTES))])
KEYS = ("token_ids", "strings", "max_new_tokens")
REASONS = ("eos", "stop_token", "stop_string", "length")
_BYTE_FALLBACK = re.compile(r"<0x([0-9a-fA-F]{2})>\Z")


# ------------------------------------------------------------------------------------------------------------------- the byte table
def token_text_bytes(token: str, text: str) -> bytes:
    """The bytes one vocabulary entry decodes to: `text` is what the tokenizer's decoder makes of `token`; a byte-fallback token
    `<0xNN>` is the single byte NN whatever the decoder says."""
    m = _BYTE_FALLBACK.match(token)
    return bytes([int(m.group(1), 16)]) if m else text.encode("utf-8")


def table_from_list(entries: Sequence[bytes]):
    """(offsets int32 [V + 1], bytes uint8) of one bytes object per id.  A token of more than 255 bytes raises ValueError."""
    lens = [len(e) for e in entries]
    if lens and max(lens) > MAX_TOKEN_BYTES:
        raise ValueError(f"token {int(np.argmax(lens))} decodes to {max(lens)} bytes; at most {MAX_TOKEN_BYTES} are supported")
    off = np.zeros(len(entries) + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer(b"".join(entries), np.uint8).copy()
    return off, (data if len(data) else np.zeros(1, np.uint8))


def token_bytes(tokenizer, vocab_size: Optional[int] = None, static_prefix: str = "abcdef"):
    """The table of a tokenizer, built once per tokenizer: entry t = the bytes id t decodes to (see the module docstring); ids the
    vocabulary does not name, up to `vocab_size`, decode to nothing."""
    vocab = tokenizer.get_vocab()
    base = tokenizer.convert_ids_to_tokens(tokenizer(static_prefix, add_special_tokens=False)["input_ids"])
    entries = [b""] * max(max(vocab.values()) + 1, int(vocab_size or 0))
    for token, idx in vocab.items():
        text = tokenizer.convert_tokens_to_string(list(base) + [token])
        entries[idx] = token_text_bytes(token, text[text.index(static_prefix) + len(static_prefix):])
    return table_from_list(entries)


def bytes_of(table, t: int) -> Optional[bytes]:
    """The bytes of id t, or None for an id outside the table."""
    if table is None:
        return None
    off, data = table
    if not 0 <= t < len(off) - 1:
        return None
    return data[int(off[t]):int(off[t + 1])].tobytes()


# ---------------------------------------------------------------------------------------------------------------------- the rules
def string_hit(h: Sequence[int], strings: Sequence[bytes], table) -> Optional[int]:
    """Rule 3 for the newest token of h: the lowest index of a string with an occurrence that ends inside t's bytes, or None."""
    tb = bytes_of(table, int(h[-1]))
    if not tb:
        return None
    front = b""
    for x in reversed(list(h[:-1])):
        if len(front) >= MAX_STRING_BYTES - 1:
            break
        xb = bytes_of(table, int(x))
        if xb is None:                                   # the text breaks here
            break
        front = xb + front
    text = front + tb
    for i, s in enumerate(strings):
        s = bytes(s)
        for end in range(len(front) + 1, len(text) + 1):
            if s and end >= len(s) and text[end - len(s):end] == s:
                return i
    return None


def fires(h: Sequence[int], record: Optional[dict], table, eos: Optional[int], batch_max_new: int) -> Optional[Tuple[str, Optional[int]]]:
    """(reason, index) if the slot stops behind the newest token of h (len(h) >= 1), else None.  record: a `check_stop` dict or None.
    index: which of token_ids / strings for those two reasons, None for the others."""
    n, t = len(h), int(h[-1])
    rec = record or {}
    if eos is not None and int(eos) >= 0 and t == int(eos):
        return "eos", None
    ids = [int(x) for x in rec.get("token_ids", ())]
    if t in ids:
        return "stop_token", ids.index(t)
    i = string_hit(h, rec.get("strings", ()), table)
    if i is not None:
        return "stop_string", i
    budget = int(rec.get("max_new_tokens", 0) or 0)
    if n >= int(batch_max_new) or (budget > 0 and n >= budget):
        return "length", None
    return None


def first_stop(h: Sequence[int], record: Optional[dict], table, eos: Optional[int], batch_max_new: int) -> Optional[int]:
    """The smallest n >= 1 such that h[:n] stops, or None: a free-running sequence h is cut to h[:n] by the record."""
    h = [int(x) for x in h]
    for n in range(1, len(h) + 1):
        if fires(h[:n], record, table, eos, batch_max_new) is not None:
            return n
    return None


def finish_reason(h: Sequence[int], record: Optional[dict], table, eos: Optional[int], batch_max_new: int):
    """(reason, stop_index) of a finished output: a pure host function of the returned ids, so the device keeps no reason array.
    (None, None) for ids that no rule ends (a slot still running, or one retired by the caller)."""
    if len(h) < 1:
        return None, None
    hit = fires([int(x) for x in h], record, table, eos, batch_max_new)
    return hit if hit is not None else (None, None)


# ------------------------------------------------------------------------------------------------------------ arguments and records
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_stop(stop: Optional[dict], batch_max_new: Optional[int] = None, table=None, need_table: bool = True) -> Optional[dict]:
    """Validated copy of one request's `stop=` argument: dict(token_ids=(), strings=(), max_new_tokens=0), any key optional (None =
    the neutral value; a single str for `strings` is one string).  Returns None for None and for a neutral dict (no ids, no strings,
    and a budget of 0 or equal to the batch's): such a request takes the path of one that never asked.  Otherwise dict(token_ids=tuple
    of int, strings=tuple of bytes, max_new_tokens=int).  ValueError: unknown keys, more than 8 ids or strings, an id that is not an
    integer in [0, 2^31), a string that is empty or longer than 64 bytes of UTF-8, a budget outside [1, batch_max_new], strings
    without a byte table (need_table)."""
    if stop is None:
        return None
    if not isinstance(stop, dict):
        raise ValueError(f"stop must be a dict with keys {KEYS} or None, got {type(stop).__name__}")
    unknown = set(stop) - set(KEYS)
    if unknown:
        raise ValueError(f"stop: unknown keys {sorted(unknown)}")
    ids = stop.get("token_ids")
    ids = [] if ids is None else ([ids] if _is_int(ids) else list(ids))
    if len(ids) > MAX_IDS or not all(_is_int(t) and 0 <= t < 2 ** 31 for t in ids):
        raise ValueError(f"stop token_ids must be at most {MAX_IDS} integers in [0, 2^31), got {ids!r}")
    strs = stop.get("strings")
    strs = [] if strs is None else ([strs] if isinstance(strs, (str, bytes)) else list(strs))
    if len(strs) > MAX_STRINGS:
        raise ValueError(f"at most {MAX_STRINGS} stop strings, got {len(strs)}")
    out = []
    for s in strs:
        if not isinstance(s, (str, bytes)):
            raise ValueError(f"a stop string must be str or bytes, got {s!r}")
        b = s.encode("utf-8") if isinstance(s, str) else bytes(s)
        if not 1 <= len(b) <= MAX_STRING_BYTES:
            raise ValueError(f"a stop string must have 1 to {MAX_STRING_BYTES} bytes of UTF-8, {s!r} has {len(b)}")
        out.append(b)
    if out and need_table and table is None:
        raise ValueError("stop strings need the tokenizer's byte table (engine.set_stop_vocab(stopping.token_bytes(tokenizer)))")
    m = stop.get("max_new_tokens")
    m = 0 if m is None else m
    if not _is_int(m) or m < 0 or (batch_max_new is not None and m > batch_max_new):
        raise ValueError(f"stop max_new_tokens must be 0 (the batch's limit) or an integer in [1, {batch_max_new}], got {m!r}")
    if batch_max_new is not None and m == batch_max_new:
        m = 0
    if not ids and not out and m == 0:
        return None
    return dict(token_ids=tuple(int(t) for t in ids), strings=tuple(out), max_new_tokens=int(m))


def per_sequence(stop, count: int, batch_max_new: Optional[int] = None, table=None, need_table: bool = True) -> Optional[List[Optional[dict]]]:
    """A call's `stop=` argument for `count` sequences: one dict for all of them, or a list with one dict or None each -> the validated
    records, or None if every one is neutral (the call is then one without the argument)."""
    if stop is None:
        return None
    if isinstance(stop, dict):
        one = check_stop(stop, batch_max_new, table, need_table)
        return None if one is None else [one] * count
    stop = list(stop)
    if len(stop) != count:
        raise ValueError(f"{len(stop)} stop records for {count} sequences")
    recs = [check_stop(s, batch_max_new, table, need_table) for s in stop]
    return None if all(r is None for r in recs) else recs


def records(stops: Sequence[Optional[dict]]) -> np.ndarray:
    """aur_stop_rules records (numpy, RECORD), one per validated `check_stop` dict; None = the neutral, all-zero record."""
    out = np.zeros(len(stops), RECORD)
    for r, s in zip(out, stops):
        if s is None:
            continue
        r["max_new_tokens"] = s.get("max_new_tokens", 0)
        ids, strs = s.get("token_ids", ()), s.get("strings", ())
        r["n_token_ids"], r["n_strings"] = len(ids), len(strs)
        r["token_ids"][:len(ids)] = ids
        for i, b in enumerate(strs):
            r["string_len"][i] = len(b)
            r["strings"][i, :len(b)] = np.frombuffer(bytes(b), np.uint8)
    return out


def from_record(rec) -> dict:
    """What the kernel makes of one raw RECORD, values the host would reject included: counts clamped into [0, 8], string lengths
    into [0, 64] (a string of length 0 matches nothing and keeps its index), a budget <= 0 = the batch's."""
    nid = min(max(int(rec["n_token_ids"]), 0), MAX_IDS)
    nstr = min(max(int(rec["n_strings"]), 0), MAX_STRINGS)
    strs = tuple(rec["strings"][i, :min(max(int(rec["string_len"][i]), 0), MAX_STRING_BYTES)].tobytes() for i in range(nstr))
    return dict(token_ids=tuple(int(t) for t in rec["token_ids"][:nid]), strings=strs, max_new_tokens=max(int(rec["max_new_tokens"]), 0))

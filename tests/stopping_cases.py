"""Cases shared by tests/test_stopping_host.py (the definition against transformers) and tests/test_gpu_stop.py (the kernel against the
definition).  No GPU, no torch."""
import functools
import os
import random

import numpy as np

from aurora_amd import stopping as ST

TINY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_tiny")
STRINGS = ["the door", ".", "next?\nA", "ss"]
N_SEEDED = 3000

# StopStringCriteria's docstring, stop string "stop": the sequences it says trigger a match, and those it says do not
DOC_FIRE = [["st", "op"], ["stop"], ["st", "opera"], ["sto", "pper"], ["las", "topper"], ["s", "to", "pped"]]
DOC_QUIET = [["stop", "at"], ["st", "op", "at"], ["st", "opera", "tion"]]


def seeded_sequences():
    """3000 sequences of 1 to 12 ids drawn from [3, 300) with random.seed(0)"""
    rng = random.Random(0)
    return [[rng.randrange(3, 300) for _ in range(rng.randint(1, 12))] for _ in range(N_SEEDED)]


@functools.lru_cache(maxsize=None)
def doc_table():
    """a vocabulary made of the docstring's tokens: (table, token -> id)"""
    words = sorted({w for seq in DOC_FIRE + DOC_QUIET for w in seq})
    return ST.table_from_list([w.encode() for w in words]), {w: i for i, w in enumerate(words)}


def doc_cases():
    """(ids, fires?) for the nine docstring examples over `doc_table`"""
    _, ids = doc_table()
    return [([ids[w] for w in seq], True) for seq in DOC_FIRE] + [([ids[w] for w in seq], False) for seq in DOC_QUIET]


@functools.lru_cache(maxsize=None)
def synthetic_table(vocab: int = 32000, seed: int = 5):
    """token lengths 1 to 16 over a 4-letter alphabet (so that short strings occur often), a few tokens of 255 bytes and a few of 0"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 17, vocab)
    lens[[7, 1000, vocab - 1]] = 255
    lens[[0, 9, 31999 % vocab]] = 0
    lens[vocab - 1] = 255
    return ST.table_from_list([bytes(rng.integers(97, 101, int(n)).astype(np.uint8)) for n in lens])


def edge_rows():
    """(history, raw RECORD, batch_max_new, tag): the edges tests/test_gpu_stop.py lists, over `edge_table`"""
    tab = edge_table()
    A, B, C, AB, LONG, EMPTY, X = 0, 1, 2, 3, 4, 5, 6                      # "a", "b", "c", "ab", "xxabcabyy", "", "x"
    OUT = len(tab[0]) - 1                                                   # the first id outside the table
    rows = []

    def add(h, stop, tag, bmax=64, raw=None):
        rec = ST.records([ST.check_stop(stop, None, tab)])[0] if raw is None else raw
        rows.append((list(h), rec, bmax, tag))
    add([AB], dict(strings=["cab"]), "history shorter than the string")
    add([C, AB], dict(strings=["cab"]), "the same string once the history holds it")
    add([LONG], dict(strings=["abcab"]), "one token longer than the string, overhanging on both sides")
    add([X, LONG], dict(strings=["xxx"]), "left overhang into the previous token")
    add([LONG, X], dict(strings=["abcab"]), "an occurrence that ends before the last token")
    add([LONG, X], dict(strings=["yyx"]), "a string that ends at the end of t")
    s64 = "".join("abc"[i % 3] for i in range(64))
    h64 = [(A, B, C)[i % 3] for i in range(64)]
    add(h64, dict(strings=[s64]), "64 bytes over 64 one-byte tokens", bmax=128)
    add([B] + h64, dict(strings=[s64]), "64 bytes, one more token in front", bmax=128)
    add(h64[1:], dict(strings=[s64]), "63 of the 64 bytes", bmax=128)
    add(h64[:-1] + [B], dict(strings=[s64]), "64 bytes, the last one wrong", bmax=128)
    add([C] + h64[1:], dict(strings=[s64]), "64 bytes, the first one wrong", bmax=128)
    add([A, B, C], dict(strings=["x", "y", "cc", "bb", "aa", "ca", "ba", "bc"]), "8 strings, only the last matches")
    add([A, B, C], dict(strings=["x", "y", "cc", "bb", "aa", "ca", "ba", "cb"]), "8 strings, none matches")
    add([], dict(strings=["a"], token_ids=[0], max_new_tokens=1), "n = 0")
    add([A, OUT, B], dict(strings=["ab"]), "an id outside the table breaks the text")
    add([A, EMPTY, B], dict(strings=["ab"]), "a token of zero bytes does not")
    add([A, B, EMPTY], dict(strings=["ab"]), "a token of zero bytes completes nothing")
    add([A, OUT], dict(strings=["a"], token_ids=[OUT]), "an id outside the table is still a stop id")
    add([A, -1], dict(strings=["a"]), "a negative id")
    add([A, 2 ** 31 - 1], dict(strings=["a"]), "the largest id")
    add([A] * 16, dict(max_new_tokens=16), "a history that fills ids_stride, budget reached", bmax=16)
    add([A] * 15 + [B], dict(strings=["ab"]), "a history that fills ids_stride, string at its end", bmax=64)
    add([A] * 15, dict(max_new_tokens=16), "budget one short")
    add([A] * 5, dict(max_new_tokens=5), "budget 5 reached")
    add([A] * 4, dict(max_new_tokens=5), "budget 5 not reached")
    add([A] * 3, None, "the batch's limit", bmax=3)
    add([A, B], dict(token_ids=[A]), "a stop id equal to h[n - 2] only")
    add([A, B], dict(token_ids=[7, 8, 9, 10, 11, 12, 13, B]), "the eighth stop id")
    # records the host would reject
    raw = np.zeros(1, ST.RECORD)[0]
    raw["n_token_ids"], raw["n_strings"], raw["max_new_tokens"] = 100, -5, -3
    raw["token_ids"] = [9, 9, 9, 9, 9, 9, 9, B]
    add([A, B], None, "n_token_ids 100 is 8, n_strings -5 is 0, budget -3 is the batch's", raw=raw.copy())
    raw = np.zeros(1, ST.RECORD)[0]
    raw["n_token_ids"], raw["n_strings"] = -1, 100
    raw["token_ids"][0] = B
    raw["string_len"] = [-4, 0, 1000, 1, 1, 1, 1, 1]
    raw["strings"][2, :] = np.frombuffer(s64.encode(), np.uint8)
    raw["strings"][3:, 0] = ord("x")
    add(h64, None, "n_token_ids -1 is 0, string_len -4 / 0 match nothing, 1000 is 64", bmax=128, raw=raw.copy())
    add([A, B], None, "the same record, nothing matches", raw=raw.copy())
    # neighbouring rows with different records over the same history
    for stop in (dict(strings=["ab"]), dict(strings=["ba"]), dict(token_ids=[AB]), dict(token_ids=[A]), None, dict(max_new_tokens=3),
                 dict(max_new_tokens=4), dict(strings=["cab", "b"])):
        add([C, A, AB], stop, f"neighbours over one history: {stop}")
    return rows


@functools.lru_cache(maxsize=None)
def edge_table():
    return ST.table_from_list([b"a", b"b", b"c", b"ab", b"xxabcabyy", b"", b"x"])

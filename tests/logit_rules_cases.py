"""Cases shared by tests/test_logit_rules_host.py (the definition against transformers and against deliberately wrong variants) and
tests/test_gpu_logit_rules.py (the kernel against the definition): (tag, fp32 row, generated history, rules dict, eos id)."""
import itertools

import numpy as np

PENALTIES = (0.8, 1.0, 1.3)
NGRAMS = (0, 1, 2, 3)
EOS = 7
POOL = (7, 5, 0, 11)                 # the tokens histories draw from: the EOS, a positive, index 0 and a negative logit ...


def make_row(vocab: int, seed: int) -> np.ndarray:
    """Logits of both signs a few units wide, with +-0 and +-inf planted on tokens the histories use (and beside them)."""
    l = (np.random.default_rng(seed).standard_normal(vocab) * 3.0).astype(np.float32)
    l[5], l[11], l[0], l[vocab - 1], l[7] = 2.75, -1.3, 0.7, -0.45, 1.9          # finite, both signs, not powers of two
    l[13], l[17], l[19], l[23] = 0.0, -0.0, np.inf, -np.inf
    l[29], l[31] = 1e-38, -3e38                                                 # /p goes subnormal, *p overflows
    return l


def histories(g: int, vocab: int):
    """(tag, history): lengths 0, 1, g - 1 and g with heavy duplication, and longer ones whose repeats sit at the window's ends."""
    out = [("n0", []), ("n1", [5]), ("n1eos", [EOS])]
    for n in sorted({max(g - 1, 0), g, 2, 3}):
        out.append((f"same{n}", [5] * n))                                       # one token n times: every candidate window matches
        out.append((f"mix{n}", [POOL[i % 2] for i in range(n)]))                # 7 5 7 5 ...
    out += [
        ("first_only", [11, 5, 0, 11]),                                         # g = 2: the only match of the tail (11) is at i = 0
        ("last_only", [0, 13, 5, 5]),                                           # g = 2: the only match of the tail (5) is at i = n - g
        ("overlap", [5, 5, 5, 7, 5, 5, 5]),                                     # overlapping matches, two different continuations
        ("specials", [13, 17, 19, 23, 29, 31, 13, 17, 19, 23, 13]),             # +-0, +-inf, tiny and huge, repeated
        ("edges", [0, vocab - 1, 0, vocab - 1, 0]),                             # ids 0 and vocab - 1
        ("eos_in", [5, EOS, 11, 5, EOS]),                                       # the EOS inside the history
        ("long", [POOL[(i * i + i // 3) % 4] for i in range(40)]),
    ]
    return out


def cases(vocabs=(320, 323)):
    out = []
    for vocab, p, g in itertools.product(vocabs, PENALTIES, NGRAMS):
        row = make_row(vocab, 100 + vocab)
        for tag, h in histories(g, vocab):
            n = len(h)
            for m in sorted({0, n, n + 1}):
                rules = dict(repetition_penalty=p, no_repeat_ngram_size=g, min_new_tokens=m)
                out.append((f"v{vocab}-p{p}-g{g}-m{m}-{tag}", row, h, rules, EOS))
    return out

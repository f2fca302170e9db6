"""The rule of jtk_batch_word_stats (include/jtokkit_amd.h) restated plainly with Python's own string functions: no code shared
with the library.  White_Space is listed here by hand (str.isspace() differs); L and N come from unicodedata."""
import re
import unicodedata

import numpy as np

WHITE_SPACE = [*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
_SPLIT = re.compile("[" + "".join(re.escape(chr(c)) for c in WHITE_SPACE) + "]+")
_FOLD = {c: c + 32 for c in range(ord("A"), ord("Z") + 1)}
OUTS = (("n_words", np.int32), ("word_chars", np.int64), ("n_alpha_words", np.int32), ("n_symbol_words", np.int32), ("symbol_word_chars", np.int64),
        ("n_hash", np.int64), ("n_ellipsis", np.int32), ("stop_mask", np.uint32), ("n_stop_hits", np.int32), ("n_lines", np.int32),
        ("n_bullet_lines", np.int32), ("n_ellipsis_lines", np.int32), ("n_terminal_lines", np.int32), ("n_short_lines", np.int32))


def stats(docs, status, stop_words, fold, short_line_chars):
    """docs: bytes each; status: the sign decides (< 0: zeros); stop_words: bytes each.  A dict of arrays by the names of OUTS."""
    r = {name: np.zeros(len(docs), dtype=dt) for name, dt in OUTS}
    for d, doc in enumerate(docs):
        if status[d] < 0:
            continue
        text = doc.decode("utf-8")
        words = [w for w in _SPLIT.split(text) if w]
        cat = lambda w: {unicodedata.category(c)[0] for c in w}
        symbol = [w for w in words if not cat(w) & {"L", "N"}]
        r["n_words"][d] = len(words)
        r["word_chars"][d] = sum(len(w) for w in words)
        r["n_alpha_words"][d] = sum("L" in cat(w) for w in words)
        r["n_symbol_words"][d] = len(symbol)
        r["symbol_word_chars"][d] = sum(len(w) for w in symbol)
        r["n_hash"][d] = text.count("#")
        r["n_ellipsis"][d] = text.count("...") + text.count("…")
        for w in words:
            b = (w.translate(_FOLD) if fold else w).encode("utf-8")
            which = [i for i, s in enumerate(stop_words) if s == b]
            r["n_stop_hits"][d] += bool(which)
            r["stop_mask"][d] |= sum(1 << i for i in which)
        lines = [x for x in (raw.strip(" \t\r") for raw in text.split("\n")) if x]
        r["n_lines"][d] = len(lines)
        r["n_bullet_lines"][d] = sum(x.startswith("•") or x.startswith("-") for x in lines)
        r["n_ellipsis_lines"][d] = sum(x.endswith("...") or x.endswith("…") for x in lines)
        r["n_terminal_lines"][d] = sum(x[-1] in '.!?"' for x in lines)
        r["n_short_lines"][d] = sum(len(x) < short_line_chars for x in lines) if short_line_chars > 0 else 0
    return r

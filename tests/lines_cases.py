"""The named cases of the line / paragraph pass (jtk_batch_line_units, jtk_batch_line_repeats), shared by the CPU tier
(test_lines_rules_cpu.py) and the GPU tier (test_lines_gpu.py).  The edges are given relative to the tile constants of
jtokkit_amd/csrc/jtk_lines_rules.h: a granule of 16 bytes (a lane), 1024 (a wave), a tile of 4096 (a workgroup), 1024 tiles to a
step of the summary scan.  A case: name, docs (bytes), route (how the batch is encoded: "ordinary", "validate" with
JTK_ENCODE_VALIDATE_UTF8, "encode" with the special-token check), seed, base (doc_index_base).  Every case is run for both
units, both TRIM values and both modes.  edges_reached() computes, from the cases and the restatement's results, which of the
edges in all_edges() a case reaches."""
import collections

import numpy as np

import lines_ref as lr

GRANULE, WAVE, TILE, STEP = 16, 1024, 4096, 1024
MIN_BUDGET = 1280
MAX_SEED = (1 << 64) - 1
WRAP_BASE = (1 << 64) - 3
SPECIAL = b"<|endoftext|>"

Case = collections.namedtuple("Case", "name docs route seed base")
COMBOS = [(unit, trim) for unit in (lr.LINE, lr.PARAGRAPH) for trim in (False, True)]


def status_of(case):
    """What the encode of `route` leaves: -6 for a document that is not UTF-8 under "validate", -2 for one that holds a special
    literal under "encode", else 0 (the GPU tier checks the device's signs against these)."""
    out = []
    for doc in case.docs:
        st = 0
        if case.route == "validate":
            try:
                doc.decode("utf-8")
            except UnicodeDecodeError:
                st = -6
        if case.route == "encode" and SPECIAL in doc:
            st = -2
        out.append(st)
    return out


def word(i, n):
    """n letters that depend on i alone: equal (i, n) give equal lines."""
    return bytes(97 + (i * 7 + j * 3) % 26 for j in range(n))


def placed(total, spans):
    """A text of `total` newlines with lines at the byte ranges `spans` [(begin, end)]: same-length lines are equal."""
    a = bytearray(b"\n" * total)
    for b, e in spans:
        a[b:e] = word(1, e - b)
    return bytes(a)


def _wrap_docs(m, want_wrap=True):
    """One document of m distinct lines and a seed under which pass 1's probe walk wraps from the last slot to slot 0."""
    doc = b"\n".join(b"w%d" % i for i in range(m))
    cap = lr.capacity(m)
    for seed in range(1, 4000):
        kd = lr.doc_key(lr.key_of(seed, lr.LINE), 0, 0)
        used, wrapped = set(), False
        for i in range(m):
            s = lr.k_of(b"w%d" % i, kd) & (cap - 1)
            while s in used:
                wrapped |= s == cap - 1
                s = (s + 1) & (cap - 1)
            used.add(s)
        if wrapped == want_wrap:
            return doc, seed
    raise AssertionError("no seed wraps")


def cases():
    out = []
    C = lambda name, docs, route="ordinary", seed=0, base=0: out.append(Case(name, list(docs), route, seed, base))
    C("empties", [b"", b"\n", b"  \t\r", b" \n \n", b"abc", b"abc\n", b"\n\nabc\n\n", b"", b"\n\n\n", b"abc\nabc", b""])
    C("crlf", [b"a\r\nb\r\na\r\n", b"p\r\nq\r\n\r\nr\r\n\r\np\r\nq", b"x\ry\rx", b"\r\n\r\n"], seed=MAX_SEED)
    C("trim_equal", [b"  foo\nfoo  \n\tfoo\t\nfoo\nf oo\nf oo \n", b"bar \nbar\n bar"], base=WRAP_BASE)
    C("blank_between", [b"p1 line\n \np2 line\n \np1 line\n", b"one\n\t\r\none\n \n \nthree\n\nthree"])
    C("newline_runs", [b"a\nb\n\nc\n\n\nd\na\n\nb\n\n\nc\nd", b"\na\n\n\nb\nc\n\n\na\n\n\nb\nc\n\n"], seed=MAX_SEED, base=WRAP_BASE)
    C("prefix_nul_ends", [b"abc\nabcd\nabc\nab\nabcd", b"\x00\n\x00\x00\n\x00\n\x00\x00\x00\n\x00\x00", b"Xbcdefgh\nYbcdefgh\nabcdefgX\nabcdefgY\nXbcdefgh\nabcdefgY",
                          b"a\nb\na\nc\nb"])
    # unit begins and ends on the first and the last byte of a granule, a wave and a workgroup
    spans = [(0, 1), (15, 16), (32, 48), (1000, 1024), (2047, 2049), (3072, 3073), (4090, 4096), (8191, 8200), (12280, 12289), (12298, 12299)]
    C("tile_edges", [placed(12300, spans), placed(37, [(0, 16), (20, 36)])])
    # a unit over three workgroups (twice, at another alignment), lines around it
    long3 = word(5, 2 * TILE + 700)
    C("long_unit", [b"head\n" + long3 + b"\nhead\n\n" + long3 + b"\ntail", b"tail\n" + long3[:-1] + b"\n" + long3[1:]], seed=7, base=11)
    # a unit over more tiles than one step of the summary scan takes (twice: the carries of both must agree)
    huge = bytes(32 if j % 8 == 7 else x for j, x in enumerate(word(9, STEP * TILE + 5000)))     # (words: a piece of 1 MiB is refused by the encode)
    C("scan_steps", [b"x\n" + huge + b"\ny\n\nx\n\n" + huge + b"\ny"], seed=3)
    # a document edge inside a granule with no newline before it; the same line at the end of d and the start of d + 1
    C("doc_edges", [b"xyz\nab", b"c\nxyz\nabc", b"same", b"same", b"q\nsame", b"same\nq", b"", b"abc\n\nabc", b"abc\n\nabc"], base=5)
    # characters of 2, 3 and 4 bytes over granule, wave and workgroup edges, stray continuation bytes
    u = bytearray(b"\n" * 4200)
    u[12:15] = b"caf"
    u[15:17] = "é".encode()
    u[1022:1025] = "€".encode()
    u[2047:2049] = "é".encode()
    u[4094:4098] = "\U0001F600".encode()
    u = u + bytearray(b"\n" * 8192)
    u[8191:8193] = "é".encode()                                  # the same over the edges of the second and third tile
    u[12286:12289] = "€".encode()
    u[100:105] = b"\x80\x80ab\xbf"
    u[200:204] = "\U0001F600".encode()
    u[300:304] = "\U0001F600".encode()
    C("utf8_edges", [bytes(u), "é\né\n€€\n".encode() + b"\x80\n\x80"])
    lines = [b"l65"] * 65 + [b"l3"] * 3 + [b"l2"] * 2 + [b"one"]
    mixed = [lines[(i * 37) % len(lines)] for i in range(len(lines))]
    C("counts", [b"\n".join(mixed), b"a\nb\na\nb\n", b"t\nx\nt\n", b"only", b"x\ny\ny", b"l2\n\nl2\n\nl3\n\nl3\n\nl3"])
    C("refused_utf8", [b"dup\ndup\n", b"dup\ndup\n\xff", b"dup\n\ndup", b"\xff"], route="validate", seed=9, base=5)
    C("refused_special", [b"dup\ndup\n", b"dup\n" + SPECIAL + b"\ndup\ndup", b"x\nx", SPECIAL], route="encode")
    for name, m in (("table_cap_64", 32), ("table_cap_128", 33)):
        doc, seed = _wrap_docs(m)
        C(name, [doc], seed=seed)
    # a group boundary between documents that share a granule (at the smallest budget: 32 units to a table), a document over the
    # budget, a group of unit-less documents
    big = b"\n".join(b"g%d" % (i % 30) for i in range(45))
    C("grouping", [b"zzzz"] + [b"a\na"] * 40 + [big, b"", b"\n", b"\n\n", big[2:]] + [b"", b" "] + [b"k\nk"] * 3)
    C("odd_offsets", [b"abc", b"de\nde", b"f", b"ghi\ng\nghi", b"\n", b"jk\n\njk\n\nj"], seed=MAX_SEED, base=0)
    return out


def all_edges():
    e = {("empty_doc",), ("newline_only_doc",), ("blank_only_doc",), ("final_newline", True), ("final_newline", False), ("crlf",),
         ("equal_after_trim",), ("blank_line_separates_under_trim",), ("newline_run", 1), ("newline_run", 2), ("newline_run", 3), ("proper_prefix",),
         ("nul_lines",), ("differ_first_byte",), ("differ_last_byte",), ("one_byte_unit",), ("unit_three_workgroups",), ("unit_over_scan_step",),
         ("doc_edge_inside_granule_without_newline",), ("same_line_end_and_start_of_neighbours",), ("stray_continuation",),
         ("count", 2), ("count", 3), ("count", 65), ("top_tie",), ("top_first_is_first_unit",), ("top_first_is_last_unit",),
         ("refused", "validate"), ("refused", "encode"), ("seed", 0), ("seed", MAX_SEED), ("base", 0), ("base", WRAP_BASE),
         ("probe_wraps", 64), ("probe_wraps", 128), ("group_boundary_inside_granule",), ("doc_over_budget",), ("unitless_group",), ("odd_doc_off",)}
    for what in ("begin", "end"):
        for size in (GRANULE, WAVE, TILE):
            e |= {(what, "first_byte_of", size), (what, "last_byte_of", size)}
    for n in (2, 3, 4):
        e |= {("char_straddles", n, GRANULE), ("char_straddles", n, WAVE), ("char_straddles", n, TILE)}
    return e


def edges_reached(case, results):
    """results: {(unit, trim, mark_first): the restatement's result}."""
    got = {("seed", case.seed), ("base", case.base)}
    docs, status = case.docs, status_of(case)
    doc_off = np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.int64)
    text = b"".join(docs)
    for d, doc in enumerate(docs):
        if not doc:
            got.add(("empty_doc",))
        elif not doc.strip(b"\n"):
            got.add(("newline_only_doc",))
        elif not doc.strip(b" \t\r"):
            got.add(("blank_only_doc",))
        elif status[d] >= 0:
            got.add(("final_newline", doc.endswith(b"\n")))
        if b"\r\n" in doc:
            got.add(("crlf",))
        for n in (1, 2, 3):
            if any(len(run) == n for run in _runs(doc, b"\n")):
                got.add(("newline_run", n))
        if status[d] < 0 and len(set(doc.split(b"\n"))) < len(doc.split(b"\n")):
            got.add(("refused", case.route))
        if d and doc_off[d] % GRANULE and docs[d - 1] and doc and not docs[d - 1].endswith(b"\n") and not doc.startswith(b"\n"):
            got.add(("doc_edge_inside_granule_without_newline",))
        if d and docs[d - 1] and doc and docs[d - 1].split(b"\n")[-1] == doc.split(b"\n")[0] != b"":
            got.add(("same_line_end_and_start_of_neighbours",))
        if doc_off[d] % 2 and doc:
            got.add(("odd_doc_off",))
        a = np.frombuffer(doc, dtype=np.uint8)
        lead = np.flatnonzero(a >= 0xC0)
        for i in lead:
            n = 2 if a[i] < 0xE0 else 3 if a[i] < 0xF0 else 4
            p = int(doc_off[d] + i)
            for size in (GRANULE, WAVE, TILE):
                if p // size != (p + n - 1) // size:
                    got.add(("char_straddles", n, size))
        cont = (a & 0xC0) == 0x80
        if len(a) and (cont[0] or (cont[1:] & (a[:-1] < 0x80)).any()):
            got.add(("stray_continuation",))
    r0, r1 = results[lr.LINE, False, False], results[lr.LINE, True, False]
    if len(r1.unit_begin) and r1.n_dup.sum() > r0.n_dup.sum():
        got.add(("equal_after_trim",))
    if len(results[lr.PARAGRAPH, True, False].unit_begin) > len(results[lr.PARAGRAPH, False, False].unit_begin) and b"\n \n" in text:
        got.add(("blank_line_separates_under_trim",))
    for (unit, trim, mark), r in results.items():
        b, e = r.unit_begin, r.unit_end
        for what, pos in (("begin", b), ("end", e - 1)):
            for size in (GRANULE, WAVE, TILE):
                if (pos % size == 0).any():
                    got.add((what, "first_byte_of", size))
                if (pos % size == size - 1).any():
                    got.add((what, "last_byte_of", size))
        if (e - b == 1).any():
            got.add(("one_byte_unit",))
        if ((e - 1) // TILE - b // TILE >= 2).any():
            got.add(("unit_three_workgroups",))
        if ((e - 1) // (TILE * STEP) > b // (TILE * STEP)).any():
            got.add(("unit_over_scan_step",))
        for d in range(len(docs)):
            lo, hi = int(r.unit_off[d]), int(r.unit_off[d + 1])
            units = [text[b[i]:e[i]] for i in range(lo, hi)] if hi - lo <= 200 else []
            counts = collections.Counter(units)
            for n in (2, 3, 65):
                if n in counts.values():
                    got.add(("count", n))
            if len(units) > 1 and sorted(counts.values())[-2:] == [r.top_count[d]] * 2 and r.top_count[d] >= 2:
                got.add(("top_tie",))
            if hi > lo and r.top_first[d] == 0 and r.top_count[d] >= 2:
                got.add(("top_first_is_first_unit",))
            if hi > lo and r.top_first[d] == hi - lo - 1:
                got.add(("top_first_is_last_unit",))
            for x in units:
                for y in units:
                    if len(x) < len(y) and y.startswith(x):
                        got.add(("proper_prefix",))
                    if len(x) == len(y) > 1 and x != y and x[1:] == y[1:]:
                        got.add(("differ_first_byte",))
                    if len(x) == len(y) > 1 and x != y and x[:-1] == y[:-1]:
                        got.add(("differ_last_byte",))
            if b"\x00" in units and b"\x00\x00" in units:
                got.add(("nul_lines",))
        if not trim and unit == lr.LINE and not mark:
            n_units = np.diff(r.unit_off).tolist()
            gs = lr.groups(n_units, MIN_BUDGET)
            for d0, d1, m in gs:
                if d0 and doc_off[d0] % GRANULE and docs[d0] and docs[d0 - 1] and m and n_units[d0 - 1]:
                    got.add(("group_boundary_inside_granule",))
                if d1 - d0 == 1 and lr.capacity(m) * 20 > MIN_BUDGET:
                    got.add(("doc_over_budget",))
                if m == 0 and d1 - d0 > 1:
                    got.add(("unitless_group",))
            if len(docs) == 1 and case.name.startswith("table_cap"):
                cap = lr.capacity(n_units[0])
                used, wrapped = set(), False
                for k in r.ks[0]:
                    s = k & (cap - 1)
                    while s in used:
                        wrapped |= s == cap - 1
                        s = (s + 1) & (cap - 1)
                    used.add(s)
                if wrapped:
                    got.add(("probe_wraps", cap))
    return got


def _runs(doc, byte):
    """The maximal runs of `byte` strictly inside the ink of a document (between two other bytes)."""
    out, run, seen_other = [], b"", False
    for x in doc:
        if x == byte[0]:
            run += byte
        else:
            if run and seen_other:
                out.append(run)
            run, seen_other = b"", True
    return out

"""Plain references of JTK_ENCODE_VALIDATE_UTF8 -- test infrastructure only.

well_formed() is CPython's strict decoder and is the reference of record: a document is well-formed exactly when
bytes.decode("utf-8") accepts it (shortest form, no surrogates, nothing above U+10FFFF, no cut sequence).

The second reference is an automaton over Unicode Table 3-7 that shares nothing with the decoder or with the rule header
(jtokkit_amd/csrc/jtk_validate_rules.h).  Its constants are the fields of a Rule, so that the CPU tier can make it wrong on
purpose -- one constant moved by one, document boundaries ignored, empty documents taking the flag -- and check that the case
set tells every such version from the right one.  Those are mutants of this reference, never of the code under test."""
import collections

BAD_UTF8 = -6

Rule = collections.namedtuple("Rule", "lead_min lead_max e0_min ed_max f0_min f4_max max_len ignore_boundaries empties_take_flag")
TABLE_3_7_RULE = Rule(lead_min=0xC2, lead_max=0xF4, e0_min=0xA0, ed_max=0x9F, f0_min=0x90, f4_max=0x8F, max_len=4,
                      ignore_boundaries=False, empties_take_flag=False)


def well_formed(doc):
    try:
        bytes(doc).decode("utf-8")
    except UnicodeDecodeError:
        return False
    return True


def statuses(docs):
    """The status of every document of a batch by the reference of record."""
    return [0 if well_formed(d) else BAD_UTF8 for d in docs]


def bad_positions(b, rule=TABLE_3_7_RULE):
    """The positions at which the automaton rejects: a byte that leads nothing (a stray continuation byte included) and the
    lead of a sequence that is cut or whose second byte is outside its row of the table.  After a rejected lead the automaton
    starts again at the next byte."""
    out = []
    i, n = 0, len(b)
    while i < n:
        c = b[i]
        if c < 0x80:
            i += 1
            continue
        if c < rule.lead_min or c > rule.lead_max or c < 0xC0:
            out.append(i)
            i += 1
            continue
        need = min(4 if c >= 0xF0 else 3 if c >= 0xE0 else 2, rule.max_len)
        lo, hi = 0x80, 0xBF
        if c == 0xE0:
            lo = rule.e0_min
        elif c == 0xED:
            hi = rule.ed_max
        elif c == 0xF0:
            lo = rule.f0_min
        elif c == 0xF4:
            hi = rule.f4_max
        ok = i + need <= n and lo <= b[i + 1] <= hi and all(0x80 <= x <= 0xBF for x in b[i + 2:i + need])
        if ok:
            i += need
        else:
            out.append(i)
            i += 1
    return out


def automaton_well_formed(doc, rule=TABLE_3_7_RULE):
    return not bad_positions(doc, rule)


def automaton_statuses(docs, rule=TABLE_3_7_RULE):
    """The status of every document of a batch by the automaton.  rule.ignore_boundaries: the automaton runs over the batch's
    text as if it were one document, and a rejected position flags the document that holds it.  rule.empties_take_flag: the
    empty documents directly in front of a document whose first byte is rejected are flagged with it."""
    out = [0] * len(docs)
    if rule.ignore_boundaries:
        bad = set(bad_positions(b"".join(docs), rule))
        pos = 0
        for d, doc in enumerate(docs):
            if any(p in bad for p in range(pos, pos + len(doc))):
                out[d] = BAD_UTF8
            pos += len(doc)
        return out
    for d, doc in enumerate(docs):
        bad = bad_positions(doc, rule)
        if not bad:
            continue
        out[d] = BAD_UTF8
        if rule.empties_take_flag and bad[0] == 0:
            e = d - 1
            while e >= 0 and not docs[e]:
                out[e] = BAD_UTF8
                e -= 1
    return out

#!/usr/bin/env python3
"""Static instruction counts per basic block of one kernel, from the compiler's assembly listing.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S jtokkit_amd/csrc/jtk_kernels.hip -o k.s
    python tools/isa_blocks.py k.s k_piece_resolve [--loops-only]

Prints every basic block of the kernel whose (mangled) name contains the given text, in layout order, with its
instruction counts by class, the blocks it can go to, and a mark on the blocks of the innermost loops; then one
line per loop with the sums over its blocks.  Classes go by mnemonic prefix only:

    valu    v_*                                  vector ALU (cross-lane moves and exec-masked compares included)
    salu    s_* that is nothing below            scalar ALU, exec-mask handling
    smem    s_load*, s_buffer_load*              scalar memory reads
    lds     ds_*                                 LDS reads, writes and atomics
    vmem    global_*, buffer_*, flat_*, scratch_*  vector memory
    wait    s_wait*, s_nop*, s_sle*, s_barr*     waits and barriers; of these, by the terms of an s_waitcnt:
    w_vm    ... with a vmcnt term                vector-memory waits (loads and, on gfx9, stores)
    w_lgkm  ... with an lgkmcnt term             LDS, scalar-memory and message waits (one s_waitcnt may count in both)
    branch  s_bra*, s_cbr*, s_setpc*, s_swap*, s_endp*

A block starts at a label and after every branch.  Counts are static: a block under an exec-mask branch counts
whether or not lanes are live in it.  Needs nothing but the listing: it runs without a GPU.
"""
import argparse
import re
import sys

CLASSES = ("valu", "salu", "smem", "lds", "vmem", "wait", "branch")
WAIT_KINDS = ("w_vm", "w_lgkm")
PREFIXES = (
    ("branch", ("s_bra", "s_cbr", "s_setpc", "s_swap", "s_endp")),
    ("wait", ("s_wait", "s_nop", "s_sle", "s_barr")),
    ("smem", ("s_load", "s_buffer_load")),
    ("lds", ("ds_",)),
    ("vmem", ("global_", "buffer_", "flat_", "scratch_")),
    ("valu", ("v_",)),
    ("salu", ("s_",)),
)
LABEL = re.compile(r"^([.\w$]+):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")


def classify(mnemonic):
    for cls, prefixes in PREFIXES:
        if mnemonic.startswith(prefixes):
            return cls
    return None


def kernel_lines(path, name):
    """The lines between the kernel's entry label and the end of its code."""
    lines = open(path).read().splitlines()
    start = None
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m and name in m.group(1) and not m.group(1).startswith("."):
            if start is not None and lines[start] != ln:
                raise SystemExit("more than one kernel matches %r: %s and %s" % (name, lines[start], ln))
            start = i
    if start is None:
        raise SystemExit("no kernel whose name contains %r in %s" % (name, path))
    for j in range(start + 1, len(lines)):
        if lines[j].startswith(".Lfunc_end") or lines[j].lstrip().startswith(".end_amdhsa_kernel"):
            return lines[start:j]
    return lines[start:]


class Block:
    def __init__(self, name):
        self.name = name
        self.counts = dict.fromkeys(CLASSES, 0)
        self.waits = dict.fromkeys(WAIT_KINDS, 0)
        self.targets = []         # labels branched to
        self.falls = True         # control can run into the next block
        self.succ = []

    @property
    def total(self):
        return sum(self.counts.values())


def blocks_of(lines):
    blocks = [Block("entry")]
    cut = False                   # the last instruction was a branch: the next one starts a block
    part = 0
    for ln in lines[1:]:
        m = LABEL.match(ln)
        if m:
            if blocks[-1].total or blocks[-1].name != "entry":
                blocks.append(Block(m.group(1)))
            else:
                blocks[-1].name = m.group(1)
            cut, part = False, 0
            continue
        m = INSN.match(ln.split(";")[0].split("//")[0])
        if not m:
            continue
        cls = classify(m.group(1))
        if cls is None:
            continue
        if cut:
            part += 1
            blocks.append(Block("%s+%d" % (blocks[-1].name.split("+")[0], part)))
            cut = False
        b = blocks[-1]
        b.counts[cls] += 1
        if m.group(1) == "s_waitcnt":
            b.waits["w_vm"] += "vmcnt" in m.group(2)
            b.waits["w_lgkm"] += "lgkmcnt" in m.group(2)
        if cls == "branch":
            cut = True
            t = m.group(2).strip()
            if t.startswith("."):
                b.targets.append(t.split()[0])
            if m.group(1).startswith(("s_bra", "s_setpc", "s_endp")):             # unconditional: nothing falls through
                b.falls = False
    index = {b.name: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        b.succ = [index[t] for t in b.targets if t in index]
        if b.falls and i + 1 < len(blocks):
            b.succ.append(i + 1)
    return blocks


def loops_of(blocks):
    """Natural loops of the back edges (an edge to a block at or before its source in layout order): header -> set of blocks."""
    pred = [[] for _ in blocks]
    for i, b in enumerate(blocks):
        for s in b.succ:
            pred[s].append(i)
    loops = {}
    for i, b in enumerate(blocks):
        for h in b.succ:
            if h > i:
                continue
            body, work = {h}, [i]
            while work:
                x = work.pop()
                if x in body or x < h:       # (x < h: not dominated by the header in a reducible layout; stay inside)
                    continue
                body.add(x)
                work.extend(pred[x])
            loops.setdefault(h, set()).update(body)
    return loops


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--loops-only", action="store_true", help="print only the blocks that lie in a loop")
    a = ap.parse_args()
    blocks = blocks_of(kernel_lines(a.listing, a.kernel))
    loops = loops_of(blocks)
    inner = {h: body for h, body in loops.items() if not any(o != h and o in body for o in loops)}
    in_loop = {}
    for h in sorted(loops, key=lambda h: -len(loops[h])):     # the smallest loop that holds a block names it
        for x in loops[h]:
            in_loop[x] = h
    head = "%-16s %5s " % ("block", "all") + " ".join("%6s" % c for c in CLASSES + WAIT_KINDS) + "  loop            to"
    print(head)
    tot = Block("kernel")
    for i, b in enumerate(blocks):
        for c in CLASSES:
            tot.counts[c] += b.counts[c]
        for c in WAIT_KINDS:
            tot.waits[c] += b.waits[c]
        if a.loops_only and i not in in_loop:
            continue
        h = in_loop.get(i)
        mark = "" if h is None else ("%s%s" % ("*" if h in inner else " ", blocks[h].name))
        print("%-16s %5d " % (b.name, b.total) + " ".join("%6d" % b.counts[c] for c in CLASSES) + " " + " ".join("%6d" % b.waits[c] for c in WAIT_KINDS) +
              "  %-15s %s" % (mark, " ".join(blocks[s].name for s in b.succ)))
    print("%-16s %5d " % ("kernel", tot.total) + " ".join("%6d" % tot.counts[c] for c in CLASSES) + " " + " ".join("%6d" % tot.waits[c] for c in WAIT_KINDS))
    print()
    print("loops (* innermost): sums over the loop's blocks")
    for h in sorted(loops):
        s = Block("")
        for x in loops[h]:
            for c in CLASSES:
                s.counts[c] += blocks[x].counts[c]
            for c in WAIT_KINDS:
                s.waits[c] += blocks[x].waits[c]
        print("%s%-15s %5d " % ("*" if h in inner else " ", blocks[h].name, s.total) + " ".join("%6d" % s.counts[c] for c in CLASSES) +
              " " + " ".join("%6d" % s.waits[c] for c in WAIT_KINDS) +
              "  %d blocks, %s .. %s" % (len(loops[h]), blocks[min(loops[h])].name, blocks[max(loops[h])].name))
    return 0


if __name__ == "__main__":
    sys.exit(main())

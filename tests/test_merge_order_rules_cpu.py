"""CPU tier: which queue entry a lane of a lean merge wave works on (jtokkit_amd/csrc/jtk_merge_order_rules.h), run on the CPU
through the stand-alone program tests/merge_order_sim, built once plainly and once with -fsanitize=address,undefined.  Windows of
every size 0..W+1 in several length patterns, with and without entries that need no merge: perm is a permutation, stable within
a length, the entries without a merge last, equal to numpy's stable argsort; the rounds of a pass at counts around every
threshold for one and four workgroups per shard.  Then the schedule model (tools/merge_schedule.py) on corpus.mixed(1000, seed=3):
the wave-steps of the 4..8-byte bin with windows of 256 against 64 consecutive entries per wave.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMAX, W, NC_MAX = 4, 256, 16
LANES = 1024                                    # JTK_ML_THREADS: entries of a workgroup pass of one round


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sim(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("merge_order_sim") / ("merge_order_sim_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", out,
                           os.path.join(ROOT, "tests", "merge_order_sim", "merge_order_sim.cpp")])

    def ask(lines):
        r = subprocess.run([out], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        got = r.stdout.splitlines()
        assert len(got) == len(lines)
        return [[int(x) for x in g.split()] for g in got]
    return ask


def test_constants(sim):
    assert sim(["const"]) == [[RMAX, W, NC_MAX]]
    # 4..8 bytes: five classes; shorter and longer lengths fall into the first and last
    assert [c[0] for c in sim(["class %d 4 5" % n for n in range(1, 12)])] == [0, 0, 0, 0, 1, 2, 3, 4, 4, 4, 4]
    assert [c[0] for c in sim(["class %d 17 16" % n for n in (16, 17, 18, 31, 32, 33)])] == [0, 0, 1, 14, 15, 15]


def _windows():
    """(R, nc, keys[64 R]) for queues of 0..W+1 entries (a window takes the first 64 R of them; what is absent has key nc)"""
    rnd = np.random.RandomState(7)
    out = []
    for R, nc in ((4, 5), (2, 5), (4, 16), (1, 5)):
        size = 64 * R
        for n in range(0, W + 2):
            m = min(n, size)
            i = np.arange(m)
            for pat in ("random", "ascending", "descending", "equal", "alternating", "one_long", "some_done"):
                if pat == "random" or pat == "some_done":
                    k = rnd.randint(0, nc, m)
                elif pat == "ascending":
                    k = i * nc // max(m, 1)
                elif pat == "descending":
                    k = (nc - 1) - i * nc // max(m, 1)
                elif pat == "equal":
                    k = np.full(m, nc // 2)
                elif pat == "alternating":
                    k = np.where(i % 2 == 0, 0, nc - 1)
                else:
                    k = np.where(i == (137 % max(m, 1)), nc - 1, 0)
                if pat == "some_done":
                    k = np.where(rnd.rand(m) < 0.3, nc, k)              # JTK_QE_DONE among pieces that merge
                keys = np.full(size, nc, dtype=np.int64)
                keys[:m] = k
                out.append((R, nc, keys))
            if n > size + 1:
                break
    return out


def test_order_of_every_window_size(sim):
    wins = _windows()
    assert len(wins) > 3000
    got = sim(["order %d %d %s" % (R, nc, " ".join(map(str, k))) for R, nc, k in wins])
    saw_done_inside = saw_partial = False
    for (R, nc, keys), g in zip(wins, got):
        size = 64 * R
        n_live, perm = g[0], np.array(g[1:])
        assert len(perm) == size and n_live == int((keys < nc).sum())
        assert np.array_equal(np.sort(perm), np.arange(size))                            # a permutation of the window
        live = perm[:n_live]
        assert (keys[live] < nc).all() and (keys[perm[n_live:]] == nc).all()             # no merge: last
        k = keys[perm]
        assert (np.diff(k) >= 0).all()                                                   # ascending
        same = np.diff(k) == 0
        assert (np.diff(perm)[same] > 0).all()                                           # stable within a length
        assert np.array_equal(perm, np.argsort(keys, kind="stable"))
        saw_done_inside |= bool((keys[:n_live] == nc).any())
        saw_partial |= 0 < n_live < size
    assert saw_done_inside and saw_partial


def _passes(sim, count, span):
    """the passes of a queue: [(first entry, R)], asking the rule before each"""
    out, taken = [], 0
    while taken < count:
        R = sim(["rounds %d %d" % (count - taken, span)])[0][0]
        out.append((taken, R))
        taken += R * span
    return out


@pytest.mark.parametrize("K", [1, 4])
def test_rounds_of_a_pass_around_every_threshold(sim, K):
    span = K * LANES
    edges = sorted({e + d for e in (0, span, 2 * span, 3 * span, 4 * span, 6 * span, 8 * span, 9 * span) for d in (-1, 0, 1) if e + d >= 0}
                   | {4 * span + r for r in (63, 64, 65, 255)})
    asked = sim(["rounds %d %d" % (n, span) for n in edges])
    for n, (R,) in zip(edges, asked):
        # R rounds only while every wave of every workgroup of the shard gets a full window of 64 R entries
        assert R == (4 if n >= 4 * span else 2 if n >= 2 * span else 1), (n, R)
    assert sim(["rounds %d %d" % (2 * span - 1, span)]) == [[1]] and sim(["rounds %d %d" % (2 * span, span)]) == [[2]]
    assert sim(["rounds %d %d" % (4 * span - 1, span)]) == [[2]] and sim(["rounds %d %d" % (4 * span, span)]) == [[4]]
    assert sim(["rounds 4294967295 %d" % span]) == [[4]]                               # no overflow in the comparison
    for n in (0, 1, span, 2 * span - 1, 2 * span + 1, 4 * span + 255, 7 * span + 5, 9 * span + 1):
        ps = _passes(sim, n, span)
        # ordered passes are whole, come first and go 4, ..., 4, 2; the rest is taken as before, in as many passes as before
        rs = [R for _, R in ps]
        assert rs == sorted(rs, reverse=True) and rs.count(2) <= 1
        for at, R in ps:
            assert R == 1 or at + R * span <= n
        ordered = sum(R * span for _, R in ps if R > 1)
        assert n - ordered < 2 * span and rs.count(1) == (n - ordered + span - 1) // span
        assert sum(rs) == (n + span - 1) // span                                     # never more rounds per wave than before


def test_schedule_model_on_mixed_text(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    import merge_schedule as ms
    from jtokkit_amd import corpus
    text, doc_off = corpus.mixed(1000, seed=3)
    rows = ms.table(ms.queues("cl100k_base", text, doc_off))
    with capsys.disabled():
        print("\n" + ms.render(rows))
    b0 = rows[0]
    assert b0["bin"] == 0 and b0["entries"] > 100000
    assert b0["no_idle"] <= b0[256] <= b0["today"]
    assert b0[256] <= 0.80 * b0["today"], (b0[256], b0["today"])

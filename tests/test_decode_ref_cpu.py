"""The plain decode reference (tests/decode_ref.py) against the CPU oracle's decodeBytes on every case of tests/decode_cases.py
and on the reference's golden rows, and the conditions that the case set must meet to reach the edges of jtk_decode.hip
(computed from decode_ref's lengths alone).  No GPU: this shows the checker of tests/test_decode_gpu.py right first."""
import base64
import ctypes as C

import numpy as np
import pytest

import decode_cases as dc
import decode_ref
import golden_util
import oracle_lib

T, S = dc.T, dc.S


def _oracle(name):
    if name != "custom":
        return oracle_lib.get(name)
    kind, ranks, specials = dc.custom_spec()
    data = b"\n".join(base64.b64encode(k) + b" " + str(v).encode() for k, v in sorted(ranks.items(), key=lambda kv: kv[1])) + b"\n"
    return oracle_lib.OracleEncoding("decode_custom", kind, data, specials)


@pytest.mark.parametrize("name", dc.TABLES)
def test_reference_equals_oracle_on_every_case(name):
    """Sequence by sequence: the oracle raises error -3 exactly where status is JTK_ERR_UNKNOWN_TOKEN, and gives the
    reference's bytes where it does not."""
    o = _oracle(name)
    L = oracle_lib.lib()
    exp = dc.expected(name)
    n_bad = 0
    for cname, ids, seq_off in dc.cases(name):
        out, byte_off, status = exp[cname]
        assert len(byte_off) == len(seq_off) and len(status) == len(seq_off) - 1 and byte_off[0] == 0 and byte_off[-1] == len(out)
        ids = np.ascontiguousarray(ids)
        buf = np.empty(max(len(out), 1), dtype=np.uint8)
        for q in range(len(seq_off) - 1):
            a, b = int(seq_off[q]), int(seq_off[q + 1])
            n = L.jtko_decode(o._h, ids.ctypes.data + 4 * a, b - a, buf.ctypes.data, len(buf))
            if status[q] != decode_ref.JTK_OK:
                assert status[q] == decode_ref.JTK_ERR_UNKNOWN_TOKEN and n == oracle_lib.ERR_UNKNOWN_TOKEN, (cname, q)
                n_bad += 1
            else:
                assert n == byte_off[q + 1] - byte_off[q] and buf[:n].tobytes() == out[byte_off[q]:byte_off[q + 1]], (cname, q)
    assert n_bad > 100


@pytest.mark.parametrize("name", golden_util.ENCODING_NAMES)
def test_reference_decodes_golden_rows_to_their_text(name):
    tab = dc.table(name)
    rows = golden_util.load_rows(name)
    ids = [i for r in rows for i in r[1]]
    seq_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])])
    out, byte_off, status = tab.decode_ref(ids, seq_off)
    assert (status == 0).all()
    for q, (inp, _, _) in enumerate(rows):
        assert out[byte_off[q]:byte_off[q + 1]] == inp.encode("utf-8"), q


def test_table_id_wins_over_special_and_lengths():
    tab = decode_ref.DecodeTable({b"a": 0, b"bc": 1, b"def": 3}, {"<s>": 1, "<hole>": 2, "<far>": 7})
    assert tab.n_table == 4 and tab.n_ids_table == 8
    assert tab.lengths([0, 1, 2, 3, 4, 7, 8, -1, 2 ** 31 - 1, -2 ** 31]).tolist() == [1, 2, 6, 3, 0, 5, 0, 0, 0, 0]
    assert tab.holes().tolist() == [4, 5, 6]
    assert {l: v.tolist() for l, v in tab.ids_by_length().items()} == {1: [0], 2: [1], 3: [3], 5: [7], 6: [2]}
    out, byte_off, status = tab.decode_ref([1, 2, 4, 0, 7, -1], [0, 2, 2, 4, 5, 6, 6])
    assert out == b"bc<hole>a<far>" and byte_off.tolist() == [0, 8, 8, 9, 14, 14, 14]
    assert status.tolist() == [0, 0, -3, 0, -3, 0]


def _tiles(tab, ids):
    """Byte sum and output offset of every tile of 2,048 tokens."""
    lens = tab.lengths(ids)
    nt = max((len(lens) + T - 1) // T, 1)
    sums = np.concatenate([lens, np.zeros(nt * T - len(lens), dtype=np.int64)]).reshape(nt, T).sum(axis=1)
    return sums, np.cumsum(sums) - sums


@pytest.mark.parametrize("name", dc.TABLES)
def test_case_set_reaches_the_edges(name):
    """Conditions on the inputs, so that a change to the builder cannot quietly lose an edge."""
    tab = dc.table(name)
    lmax = max(tab.ids_by_length())
    assert lmax == (300 if name == "custom" else 128)
    sums_seen = set()
    staged_res, direct_res = set(), set()
    small_between_full = set()
    direct_between_staged = staged_between_direct = False
    unknown_after_run, unknown_before_run, runs_at_n_tok = set(), set(), set()
    n_cases = 0
    for cname, ids, seq_off in dc.cases(name):
        n_cases += 1
        n = len(ids)
        sums, obase = _tiles(tab, ids)
        sums_seen |= set(sums.tolist())
        for i, (sm, ob) in enumerate(zip(sums.tolist(), obase.tolist())):
            if sm > S:
                direct_res.add((ob % 4, (ob + sm) % 4))
            elif sm >= 1024:                                              # (every thread of the block stores whole words)
                staged_res.add((ob % 4, (ob + sm) % 4))
            if 0 < i < len(sums) - 1:
                before, after = sums[i - 1], sums[i + 1]
                if sm <= 5 and 1024 <= before <= S and 1024 <= after <= S:
                    small_between_full.add(sm)
                if sm > S and 1024 <= before <= S and 1024 <= after <= S:
                    direct_between_staged = True
                if 1024 <= sm <= S and before > S and after > S:
                    staged_between_direct = True
        known = tab.lengths(ids) > 0
        empty = (np.diff(seq_off) == 0).tolist() + [False]
        q = 0
        while q < len(empty):                                             # maximal runs of empty sequences
            if not empty[q]:
                q += 1
                continue
            q0 = q
            while empty[q]:
                q += 1
            p, run = int(seq_off[q0]), q - q0
            if p == n and n > 0:
                runs_at_n_tok.add(run)
            if 0 < p < n:
                if not known[p]:
                    unknown_after_run.add(run)
                if not known[p - 1]:
                    unknown_before_run.add(run)
    assert {S - 1, S, S + 1, T * 128, T * lmax} <= sums_seen
    pairs = {(a, b) for a in range(4) for b in range(4)}
    assert staged_res == pairs and direct_res == pairs
    assert small_between_full == {0, 1, 2, 3, 4, 5}
    assert direct_between_staged and staged_between_direct
    assert {1, 2, 65} <= unknown_after_run and {1, 2, 65} <= unknown_before_run
    assert {1, 2, 65} <= runs_at_n_tok
    assert sum(dc.is_fuzz(c[0]) for c in dc.cases(name)) == dc.FUZZ_ROUNDS
    assert n_cases == len({c[0] for c in dc.cases(name)})

"""CPU: which senders each workgroup of the fused edge kernels lists, restated in plain Python, and -- from that model and the
plan ``ops.edge_plan`` makes today -- that every case of tests/edge_list_cases.py still contains what it is there for.  If a
change to the chunk plan moves a case off its path, this file says so; the GPU tests do not quietly stop covering it."""
import pytest

import edge_list_cases as E

LIST_MAX, LIST_MAX_Q = 160, 116   # F2_LIST_MAX / B2_LIST_MAX, B2_LIST_MAX_Q (csrc/edge_fwd2_impl.h, csrc/edge_bwd2_impl.h)


def whole_mode(N, edge_scalars=False, direction="fwd"):
    return N <= (LIST_MAX_Q if (edge_scalars and direction == "bwd") else LIST_MAX)


def shares(mask_row, N, SC, skip_masked=True, edge_scalars=False, direction="fwd"):
    """The senders each of the SC workgroups of one (jet, receiver block) lists, in list order.  ``mask_row``: N entries of 0 / 1,
    or None for a call without a mask.  The forward lists every sender when ``skip_masked`` is off or there is no mask; the
    backward always lists the unmasked ones only."""
    def listed(j):
        if mask_row is None or (direction == "fwd" and not skip_masked):
            return True
        return mask_row[j] != 0
    if whole_mode(N, edge_scalars, direction):
        lst = [j for j in range(N) if listed(j)]
        n = len(lst)
        per = -(-n // SC)
        return [lst[min(n, sc * per):][:per] for sc in range(SC)]
    JC = -(-N // SC)
    return [[j for j in range(sc * JC, min(N, sc * JC + JC)) if listed(j)] for sc in range(SC)]


def _rows(case):
    return [[1 if j in set(s) else 0 for j in range(case.N)] for s in case.sets]


def test_model_on_the_worked_examples():
    # n = 1, 2 or 4 unmasked senders cut into 3 parts: the third is empty; n = 5 fills all three
    for n, want in ((1, [[0], [], []]), (2, [[0], [1], []]), (4, [[0, 1], [2, 3], []]), (5, [[0, 1], [2, 3], [4]])):
        row = [1] * n + [0] * (30 - n)
        assert shares(row, 30, 3) == want
        assert shares(row, 30, 3, direction="bwd") == want
    assert shares([0] * 30, 30, 3) == [[], [], []]
    # the forward with skip_masked off, or without a mask, lists everyone; the backward never does
    assert shares([0] * 30, 30, 3, skip_masked=False) == [list(range(10)), list(range(10, 20)), list(range(20, 30))]
    assert shares(None, 5, 2) == [[0, 1, 2], [3, 4]]
    assert shares([0] * 30, 30, 3, skip_masked=False, direction="bwd") == [[], [], []]
    # index mode: the chunk's own range; with edge scalars the backward switches at 116 already
    row = [0] * 161
    row[160] = row[3] = 1
    assert shares(row, 161, 18) == [[3]] + [[]] * 16 + [[160]]
    assert whole_mode(120, True, "fwd") and not whole_mode(120, True, "bwd") and whole_mode(116, True, "bwd")
    assert whole_mode(160) and not whole_mode(161)


@pytest.mark.parametrize("name", sorted(E.cases()))
def test_shares_partition_the_list(name):
    """Model sanity on every case: the shares are disjoint, in order, and together the listed senders."""
    c = E.cases()[name]
    SC = E.plan(c.B, c.N).SC
    for row in _rows(c):
        for direction in ("fwd", "bwd"):
            for skip in (True, False):
                sh = shares(row, c.N, SC, skip_masked=skip, direction=direction)
                flat = [j for s in sh for j in s]
                every = direction == "fwd" and not skip
                assert flat == [j for j in range(c.N) if every or row[j]]
                assert len(sh) == SC


@pytest.mark.parametrize("name", sorted(E.cases()))
def test_case_contains_what_it_is_there_for(name):
    c = E.cases()[name]
    p = E.plan(c.B, c.N)
    rows = _rows(c)
    assert len(c.sets) == c.B and all(tuple(sorted(set(s))) == tuple(s) and (not s or (0 <= s[0] and s[-1] < c.N)) for s in c.sets)
    assert p.RB == (c.N + 31) // 32
    for what in c.there_for:
        if what == "empty_share":
            assert whole_mode(c.N)
            for direction in ("fwd", "bwd"):
                assert any(not s for row in rows for s in shares(row, c.N, p.SC, direction=direction)), (name, direction)
        elif what == "tickets":
            assert p.SC > 1 and p.tickets
        elif what == "one_receiver":
            assert c.N - 32 * (p.RB - 1) == 1 and p.RB > 1
        elif what == "index_mode":
            assert not whole_mode(c.N) and -(-c.N // p.SC) <= LIST_MAX
        elif what == "masked_chunk":
            assert not whole_mode(c.N)
            for direction in ("fwd", "bwd"):
                assert any(not s for row in rows for s in shares(row, c.N, p.SC, direction=direction)), (name, direction)
        elif what == "uneven_chunk":
            sizes = [hi - lo for lo, hi in E.chunk_bounds(c.N, p.SC)]
            assert 0 < sizes[-1] < sizes[0]
        else:
            raise AssertionError(what)


def test_cases_hold_the_masks_they_describe():
    cs = E.cases()
    a = cs["A_empty_beside_full"]
    assert [len(s) for s in a.sets] == [0, 30, 1, 8] and a.sets[2] == (29,)
    assert all(len(s) == 0 for s in cs["B_no_sender"].sets)
    d = cs["D16_n150"]
    assert [len(s) for s in d.sets[:12]] == [0, 1, 2, 4, 5, 150] * 2 and all(len(s) >= 1 for s in d.sets[12:])
    assert d.sets[3] == (0, 1, 2, 3) and d.sets[9] == (146, 147, 148, 149)
    assert [len(s) for s in cs["D2_n150"].sets] == [1, 16]
    # index mode, from the plan's own chunk bounds
    e = cs["E161_index_mode"]
    cb = E.chunk_bounds(161, E.plan(2, 161).SC)
    assert e.sets[0] == tuple(range(*cb[-1])) and len(e.sets[0]) > 0
    hole = sorted(set(range(161)) - set(e.sets[1]))
    assert hole == list(range(*cb[len(cb) // 2])) and 0 < len(hole) < 161
    e = cs["E192_index_mode"]
    cb = E.chunk_bounds(192, E.plan(2, 192).SC)
    assert e.sets[0] == () and len(e.sets[1]) == len(cb)
    assert all(sum(lo <= j < hi for j in e.sets[1]) == 1 for lo, hi in cb)
    # the filled variants: the same shape, one particle where there was none, every other jet untouched
    for name in ("A_empty_beside_full", "D16_n150"):
        c, f = cs[name], E.one_particle_instead_of_none(cs[name])
        assert (f.B, f.N) == (c.B, c.N) and any(not s for s in c.sets)
        assert all((len(t) == 1) if not s else (t == s) for s, t in zip(c.sets, f.sets))
    m = E.mask_of(a)
    assert m.shape == (4, 30, 1) and m.sum() == 39 and m[2, 29, 0] == 1 and m[0].sum() == 0

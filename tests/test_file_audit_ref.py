"""CPU checks of the file audit's yardstick (tests/file_audit_ref.py) -- one
hand-worked table, and a plain double loop over random tables -- and of the
two entry points at the library boundary, which need no device."""
import ctypes as C

import numpy as np
import pytest

from file_audit_ref import BINS, FileAuditRef, assert_audit_equal, file_audit_ref, file_select_ref

N, R = 12, 4
# members 3, 7 and 9 are not available
AVAIL = np.array([m not in (3, 7, 9) for m in range(N)])
REP = np.array([
    [0, 1, 2, 4],     # 0: all four working
    [3, 7, 5, 9],     # 1: w = 1, the copy on 5 is the last one
    [3, 7, 9, 3],     # 2: w = 0 (and 3 named twice)
    [0, 1, 2, 4],     # 3: absent (ver -1): counts nowhere
    [6, -1, 8, 10],   # 4: a hole, w = 3
    [2, 2, 3, 11],    # 5: 2 named twice: load once, w counts both slots -> 3
    [1, 3, 7, 9],     # 6: w = 1, the copy on 1 is the last one
    [5, 6, 7, 8],     # 7: w = 3
], np.int32)
VER = np.array([1, 2, 1, -1, 3, 1, 1, 4], np.int32)


def hand():
    hist = np.zeros(BINS, np.int64)
    hist[[0, 1, 3, 4]] = [1, 2, 3, 1]
    load = np.array([1, 2, 2, 4, 1, 2, 2, 4, 2, 3, 1, 1], np.int32)
    sole = np.zeros(N, np.int32)
    sole[[1, 5]] = 1
    return hist, load, sole


def test_hand_table():
    hist, load, sole = hand()
    # a master list of 4 members with R = 4: three can be drawn. File 2 needs
    # four new members; file 6 needs three and already holds 1, one of the three
    got = file_audit_ref(REP, VER, AVAIL, N, cand=[0, 1, 2, 4])
    assert_audit_equal(got, FileAuditRef(7, hist, 2, load, sole), "hand table")
    assert got.working_hist[:R].sum() == 6 and got.load[2] == 2 and got.sole.sum() == got.working_hist[1]
    # list order: with 1 as the last candidate file 6's copy is outside the pool
    assert file_audit_ref(REP, VER, AVAIL, N, cand=[0, 2, 4, 1]).starved == 1
    assert file_audit_ref(REP, VER, AVAIL, N, cand=[1, 2, 4, 0]).starved == 2
    # one candidate (Intn(0)) or none: every under-replicated file starves
    assert file_audit_ref(REP, VER, AVAIL, N, cand=[0]).starved == 6
    assert file_audit_ref(REP, VER, AVAIL, N, cand=[]).starved == 6
    assert file_audit_ref(REP, VER, AVAIL, N).starved == 0
    # everybody available: nothing to repair, nobody is a sole holder; load does not move
    full = file_audit_ref(REP, VER, np.ones(N, bool), N, cand=[0, 1, 2, 4])
    assert full.working_hist[3] == 1 and full.working_hist[4] == 6 and full.sole.sum() == 0  # (file 4's hole)
    np.testing.assert_array_equal(full.load, load)


def test_hand_select():
    sel = lambda **kw: file_select_ref(REP, VER, AVAIL, N, **kw).tolist()  # noqa: E731
    assert sel() == [0, 1, 2, 4, 5, 6, 7]
    assert sel(max_working=0) == [2]
    assert sel(max_working=1) == [1, 2, 6]
    assert sel(max_working=R - 1) == [1, 2, 4, 5, 6, 7]
    assert sel(max_working=R) == sel(max_working=8) == sel()
    assert sel(member=3) == [1, 2, 5, 6]          # file 3 names nobody: it is absent
    assert sel(member=2) == [0, 5] and sel(member=0) == [0]
    assert sel(member=5, max_working=1) == [1]    # lost if 5 died
    assert sel(member=3, cap=2) == [1, 2] and sel(cap=0) == []
    out = file_select_ref(REP, VER, AVAIL, N)
    assert out.dtype == np.int32


def loop_audit(rep, ver, avail, n, cand):
    F, r = rep.shape
    hist, load, sole = [0] * BINS, [0] * n, [0] * n
    files = starved = 0
    for f in range(F):
        if ver[f] < 0:
            continue
        files += 1
        w = in_pool = 0
        seen, one = set(), None
        for q in range(r):
            a = int(rep[f][q])
            if not 0 <= a < n:
                continue
            if a not in seen:
                seen.add(a)
                load[a] += 1
            if avail[a]:
                w += 1
                one = a
                in_pool += a in cand[:-1]
        hist[w] += 1
        if w == 1:
            sole[one] += 1
        if w < r and (len(cand) <= 1 or (len(cand) - 1) - in_pool < r - w):
            starved += 1
    return FileAuditRef(files, np.array(hist, np.int64), starved, np.array(load, np.int32), np.array(sole, np.int32))


@pytest.mark.parametrize("r", [1, 3, 4, 8])
def test_against_double_loop(r):
    rng = np.random.default_rng(100 + r)
    n, F = 23, 300
    for trial in range(6):
        rep = rng.integers(-1, n, (F, r)).astype(np.int32)
        ver = rng.integers(-1, 3, F).astype(np.int32)
        avail = rng.random(n) < 0.5
        cand = rng.permutation(n)[: rng.integers(0, min(n, r + 3))].tolist()
        assert_audit_equal(file_audit_ref(rep, ver, avail, n, cand), loop_audit(rep, ver, avail, n, cand),
                           f"R={r} trial {trial}")
        for member, mw in ((-1, 0), (-1, r - 1), (5, 8), (5, 1)):
            want = [f for f in range(F) if ver[f] >= 0 and (member < 0 or member in rep[f])
                    and (mw >= r or sum(bool(0 <= a < n and avail[a]) for a in rep[f]) <= mw)]
            assert file_select_ref(rep, ver, avail, n, member, mw).tolist() == want


# ---- the library boundary (no device needed) -----------------------------
@pytest.fixture(scope="module")
def abi():
    from gossipsim import _abi
    _abi.load()
    return _abi


def test_library_exports_and_binds(abi):
    lib = C.CDLL(str(abi.LIB_PATH))
    bound = {n for n, _, _ in abi.SYMBOLS}
    for name in ("gh_file_audit", "gh_file_select"):
        assert hasattr(lib, name), name
        assert name in bound, name
    assert abi.GH_AVAIL_ALIVE == -1 and abi.GH_AUDIT_BINS == BINS
    import gossipsim
    assert gossipsim.FileAudit._fields == FileAuditRef._fields
    assert gossipsim.GH_AVAIL_ALIVE == -1 and gossipsim.GH_AUDIT_BINS == BINS


def test_null_handle_is_refused(abi):
    lib = abi.load()
    n_out = C.c_int64(-7)
    out = (C.c_int32 * 4)()
    assert lib.gh_file_audit(None, abi.GH_AVAIL_ALIVE, None, None, None, None, None) == abi.GH_EINVAL
    assert lib.gh_file_select(None, abi.GH_AVAIL_ALIVE, -1, 8, out, 4, C.byref(n_out)) == abi.GH_EINVAL
    assert n_out.value == -7

"""The yardstick of gh_file_audit / gh_file_select: the audit of an exported
file table in numpy.

file_audit_ref(rep, ver, avail, n, cand) takes what export_files returns
(rep [F][R], ver [F]), the availability set as a bool vector over the N
members (an observer's row `hb[o] >= 0`, or export_state's alive vector), and
the master's candidate list in list order (lsm(master) ids; None: `starved`
is not computed), and follows the definitions of include/gossiphip.h word for
word. It shares no code with the engine."""
from collections import namedtuple

import numpy as np

BINS = 9
FIELDS = ("files", "working_hist", "starved", "load", "sole")
FileAuditRef = namedtuple("FileAuditRef", FIELDS)


def _working(rep, avail, n):
    """[F][R] bool: the slot names a member of the availability set."""
    rep = np.asarray(rep, np.int64)
    valid = (rep >= 0) & (rep < n)
    a = np.asarray(avail).astype(bool)
    assert a.shape == (n,)
    return valid & a[np.where(valid, rep, 0)], valid, rep


def file_audit_ref(rep, ver, avail, n, cand=None):
    work, valid, rep = _working(rep, avail, n)
    F, R = rep.shape
    exists = np.asarray(ver) >= 0
    w = work.sum(1)
    hist = np.bincount(w[exists], minlength=BINS).astype(np.int64)
    # load: a member named in several slots of a file counts once
    named = np.zeros((F, n), bool)
    fi = np.broadcast_to(np.arange(F)[:, None], rep.shape)
    named[fi[valid], rep[valid]] = True
    load = named[exists].sum(0).astype(np.int32)
    # sole: the member of the one working slot
    one = exists & (w == 1)
    sole = np.bincount(rep[one][work[one]], minlength=n).astype(np.int32)
    starved = 0
    if cand is not None:
        cand = [int(c) for c in cand]
        M = len(cand)
        pool = np.zeros(n, bool)
        pool[cand[:-1]] = True  # Intn(M - 1): the last candidate is never drawn
        in_pool = (work & pool[np.where(valid, rep, 0)]).sum(1)
        under = exists & (w < R)
        starved = int((under & ((M <= 1) | ((M - 1) - in_pool < R - w))).sum())
    return FileAuditRef(int(exists.sum()), hist, starved, load, sole)


def file_select_ref(rep, ver, avail, n, member=-1, max_working=8, cap=None):
    work, _, rep = _working(rep, avail, n)
    ok = np.asarray(ver) >= 0
    if member >= 0:
        ok &= (rep == member).any(1)
    if max_working < rep.shape[1]:
        ok &= work.sum(1) <= max_working
    out = np.flatnonzero(ok).astype(np.int32)
    return out if cap is None else out[:cap]


def assert_audit_equal(got, want, msg="", starved=True):
    """Exact equality of all five outputs, types and dtypes included."""
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        if name in ("files", "starved"):
            assert isinstance(a, int) and isinstance(b, int), f"{msg} {name}: {type(a)} / {type(b)}"
            if name == "files" or starved:
                assert a == b, f"{msg} {name}: {a} != {b}"
            continue
        assert a.dtype == b.dtype, f"{msg} {name}: dtype {a.dtype} != {b.dtype}"
        np.testing.assert_array_equal(a, b, err_msg=f"{msg} {name}")

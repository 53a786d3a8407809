"""The yardstick of gh_groups: groups and view digests of an exported state
in numpy, with a small union-find (no scipy).

groups_ref(hb, alive) takes what export_state returns ([N][N] hb, [N] alive)
and returns (group, digest, n_groups) as include/gossiphip.h defines them:
edges "running i lists running c" (i != c), weak components labelled by their
lowest member id, -1 for stopped members; digest[i] = sum mod 2^64 of mix(c)
over the members row i lists (its own entry and stopped members included), 0
for a stopped row."""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1


def mix(c):
    """mix(c) of gh_groups on a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = (np.asarray(c, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mix_int(c):
    """The same on a Python int (the check of mix itself)."""
    z = ((c + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def groups_ref(hb, alive):
    hb = np.asarray(hb)
    n = hb.shape[0]
    run = np.asarray(alive).astype(bool)
    listed = hb >= 0
    mx = mix(np.arange(n))
    digest = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        for lo in range(0, n, 1024):  # (row blocks: the product is [rows][N] uint64)
            digest[lo:lo + 1024] = (listed[lo:lo + 1024] * mx[None, :]).sum(1, dtype=np.uint64)
    digest[~run] = 0
    edge = listed & run[:, None] & run[None, :]
    np.fill_diagonal(edge, False)
    # union-find in its quick-find form (root[] always flat, so a whole row is
    # one numpy step): row i and the members it lists become one set, whose
    # root is the lowest id in it
    root = np.arange(n)
    for i in np.flatnonzero(run):
        rs = root[edge[i]]
        if rs.size == 0 or (rs[0] == root[i] and (rs == rs[0]).all()):
            continue
        rs = np.unique(np.append(rs, root[i]))
        root[np.isin(root, rs)] = rs[0]
    group = np.where(run, root, -1).astype(np.int32)
    n_groups = int((group == np.arange(n)).sum())
    return group, digest, n_groups


def sizes(group):
    """Sorted member counts of the groups."""
    _, cnt = np.unique(group[group >= 0], return_counts=True)
    return sorted(cnt.tolist())


def n_views(group, digest):
    return int(np.unique(digest[group >= 0]).size)


def assert_groups_equal(got, ref, msg=""):
    """got: an engine's Groups (or any (group, digest, n_groups, ...)); ref:
    groups_ref's tuple. Exact; `passes` is no part of it."""
    np.testing.assert_array_equal(np.asarray(got[0]), ref[0], err_msg=f"group {msg}")
    np.testing.assert_array_equal(np.asarray(got[1]).astype(np.uint64), ref[1], err_msg=f"digest {msg}")
    assert int(got[2]) == ref[2], f"n_groups {got[2]} != {ref[2]} {msg}"


# ---- scenarios (shared by the CPU checks of non-vacuity and the GPU tests) ----
def split_case(n, t_fail, t_cleanup, seed, sizes, rounds, heal=None, k=4, split=3):
    """A pull-mode split from a full start (partition_ref.pull_case with its own
    T_cleanup): the sides come into force before round `split` and are healed
    before round `heal` (None: never)."""
    from partition_ref import sides_of
    return dict(n=n, cfg=dict(fanout=k, t_fail=t_fail, t_cleanup=t_cleanup, seed=seed),
                side=sides_of(n, sizes, seed ^ 0x51DE), split=split, heal=heal, rounds=rounds, sched={}, loss=None)


CASE_A = lambda: split_case(1000, 16, 30, 0x5EED2267, [300], 50, heal=40)  # noqa: E731
CASE_B = lambda: split_case(263, 16, 30, 0x5EED2266, [90, 40], 28, heal=24)  # noqa: E731
CASE_C = lambda: split_case(263, 6, 6, 0x5EED0A01, [100, 40], 20)  # noqa: E731


def drive(case, target, per_round, rounds=None):
    """Runs the case on `target` (a PartitionModel or an Engine: set_partition,
    apply_events, step); per_round(r) after every round."""
    for r in range(1, (rounds or case["rounds"]) + 1):
        if r == case["split"]:
            target.set_partition(case["side"])
        if r == case.get("heal"):
            target.set_partition(None)
        if case["sched"].get(r):
            target.apply_events(case["sched"][r])
        target.step(1)
        per_round(r)


def side_groups(case, alive=None):
    """The group labels the sides themselves would give (lowest id per side)."""
    side = np.asarray(case["side"])
    low = {s: int(np.flatnonzero(side == s)[0]) for s in np.unique(side)}
    g = np.array([low[s] for s in side], np.int32)
    return g if alive is None else np.where(np.asarray(alive).astype(bool), g, -1).astype(np.int32)

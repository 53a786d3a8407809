"""CPU checks of the groups yardstick (tests/groups_ref.py) on hand-built
graphs with known answers, and of the scenarios tests/test_gpu_groups.py
runs on the engine: by the partition model alone (partition_ref.
PartitionModel) a healed split stays split, views diverge on the way there,
and short timeouts shatter the cluster -- so the GPU tests compare more than
one group. The NULL-handle path of gh_groups needs no device."""
import ctypes as C

import numpy as np

import groups_ref as gr
import partition_ref as pr


def _state(n, listed, alive=None):
    hb = np.full((n, n), -1, np.int32)
    for i, cs in listed.items():
        hb[i, list(cs)] = 5
    return hb, np.ones(n, np.uint8) if alive is None else np.asarray(alive, np.uint8)


def test_mix_matches_its_definition():
    ids = [0, 1, 2, 262, 65535, 2**31 - 2]
    assert [int(x) for x in gr.mix(np.array(ids))] == [gr.mix_int(c) for c in ids]
    assert len({gr.mix_int(c) for c in range(4096)}) == 4096


def test_hand_built_graphs():
    n = 12
    # 0 -> 1 -> 2 (a path, one-way listings), 3 <-> 4, 5 alone (lists itself only), 6 lists nobody;
    # 7 and 8 both list the stopped 9 (no bridge); stopped 10 lists everybody (no edges); 11 listed by 8 only
    listed = {0: [0, 1], 1: [2], 2: [2], 3: [3, 4], 4: [3, 4], 5: [5], 7: [7, 9], 8: [8, 9, 11], 10: range(n), 11: [11]}
    alive = np.ones(n, np.uint8)
    alive[[9, 10]] = 0
    hb, alive = _state(n, listed, alive)
    hb[0, 5] = -2  # a tombstone is no edge
    group, digest, ng = gr.groups_ref(hb, alive)
    assert group.tolist() == [0, 0, 0, 3, 3, 5, 6, 7, 8, -1, -1, 8]
    assert ng == 6
    assert gr.sizes(group) == [1, 1, 1, 2, 2, 3]
    m = gr.mix_int
    assert int(digest[0]) == (m(0) + m(1)) & gr.M64
    assert int(digest[8]) == (m(8) + m(9) + m(11)) & gr.M64  # the stopped member it still lists counts
    assert int(digest[6]) == 0 and int(digest[10]) == 0 and int(digest[9]) == 0
    assert int(digest[3]) == int(digest[4])  # equal views
    assert gr.n_views(group, digest) == 8  # ten running rows; 3 and 4 agree, and 1 and 2 (both list 2 alone)


def test_ref_against_a_plain_search():
    """Random sparse directed graphs: the union-find against a breadth-first
    search over the symmetrised edges."""
    rng = np.random.default_rng(11)
    for n, p in ((40, 0.03), (97, 0.012), (64, 0.2)):
        hb = np.where(rng.random((n, n)) < p, 3, rng.choice([-1, -2], (n, n))).astype(np.int32)
        alive = (rng.random(n) < 0.8).astype(np.uint8)
        group, _, ng = gr.groups_ref(hb, alive)
        run = alive.astype(bool)
        adj = (hb >= 0) & run[:, None] & run[None, :]
        adj |= adj.T
        want = np.full(n, -1, np.int32)
        for s in range(n):
            if not run[s] or want[s] >= 0:
                continue
            todo, want[s] = [s], s
            while todo:
                for c in np.flatnonzero(adj[todo.pop()]):
                    if want[c] < 0:
                        want[c] = s
                        todo.append(int(c))
        np.testing.assert_array_equal(group, want)
        assert ng == len(set(want[want >= 0].tolist()))


def _run(case, rounds=None):
    m = pr.model_of(case)
    out = {}

    def see(r):
        g, d, ng = gr.groups_ref(m.hb, m.alive)
        out[r] = (g, ng, gr.n_views(g, d))
    gr.drive(case, m, see, rounds)
    return out


def test_case_a_healed_split_stays_split():
    """N=1,000, T_fail=16, T_cleanup=30, 300 members cut off before round 3
    and healed before round 40: one group through round 19, then exactly the
    two sides, also after the heal; the views diverge on the way."""
    case = gr.CASE_A()
    out = _run(case)
    assert all(out[r][1] == 1 for r in range(1, 20))
    want = gr.side_groups(case)
    for r in range(20, 51):
        np.testing.assert_array_equal(out[r][0], want, err_msg=f"round {r}")
        assert out[r][1] == 2 and gr.sizes(out[r][0]) == [300, 700]
    assert out[18][2] == 193 and out[19][2] == 712  # distinct views (> 100)


def test_case_b_three_sides():
    case = gr.CASE_B()
    out = _run(case)
    assert out[19][1] == 1
    want = gr.side_groups(case)
    for r in range(20, 29):
        np.testing.assert_array_equal(out[r][0], want, err_msg=f"round {r}")
        assert gr.sizes(out[r][0]) == [40, 90, 133]


def test_case_c_shatters():
    """T_fail = T_cleanup = 6: the cluster falls into fragments."""
    out = _run(gr.CASE_C())
    assert out[6][1] == 1
    assert out[15][1] == 235 and out[20][1] == 235  # (> 200)
    assert sum(1 for s in gr.sizes(out[15][0]) if s > 1) >= 2


def test_groups_null_handle_is_einval():
    """A NULL handle is refused before any device is touched."""
    from gossipsim import _abi
    lib = _abi.load()
    ng, ps = C.c_int64(), C.c_int32()
    assert lib.gh_groups(None, None, None, C.byref(ng), C.byref(ps)) == _abi.GH_EINVAL

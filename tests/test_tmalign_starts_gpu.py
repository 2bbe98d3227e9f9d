"""fd_tm_align_ex on the device: starts = 3 bit for bit fd_tm_align on its parity set; all five starts and each new
start alone against the numpy restatement (tests/tmalign_starts_reference.py) in score, map and per-start scores; the
returned transform and map recomputed on the host; more starts never lower; invariance; independence of the other
pairs of a call; max_tm_across_refs with all starts.  Needs an MI355X:  pytest -m gpu"""
import ctypes as C
import json

import numpy as np
import pytest

import tm_reference as tr
import tmalign_reference as ta
import tmalign_starts_reference as ts
from foldingdiff_amd import _binding, structures

pytestmark = pytest.mark.gpu


def _record(name, **kw):
    """Print a measured value (shown with ``pytest -s``)."""
    print(f"{name}: " + json.dumps({k: float(v) for k, v in kw.items()}, sort_keys=True))


def _norm(case):
    return len(case[2]) if case[3] is None else case[3]


def _align(cases, starts, **kw):
    """The cases aligned on the device, one call per max_iter: (tm, R, t, maps, start_tms), lists in case order."""
    n = len(cases)
    out = [np.zeros(n), [None] * n, [None] * n, [None] * n, np.zeros((n, 5))]
    for it in sorted({c[4] for c in cases}):
        idx = [k for k, c in enumerate(cases) if c[4] == it]
        got = structures.tm_align([cases[k][1] for k in idx], [cases[k][2] for k in idx], norm_lens=[_norm(cases[k]) for k in idx],
                                  max_iter=it, return_transform=True, return_map=True, starts=starts, return_start_tms=True, **kw)
        for q, k in enumerate(idx):
            out[0][k], out[1][k], out[2][k], out[3][k], out[4][k] = got[0][q], got[1][q], got[2][q], got[3][q], got[4][q]
    return out


@pytest.fixture(scope="module")
def all_starts(gpu):
    return _align(ts.parity_set(), "all")


@pytest.fixture(scope="module")
def two_starts(gpu):
    return _align(ts.parity_set(), ("threading", "ss"))


def test_starts_3_is_fd_tm_align_bit_for_bit(gpu):
    """fd_tm_align_ex(starts = 3) on the 41 pairs of fd_tm_align's parity set: TM, transform, n_ali and map are the
    bytes fd_tm_align returns, and the per-start scores hold the result."""
    lib = _binding.load()
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    cases = ta.parity_set()
    for it in sorted({c[4] for c in cases}):
        sub = [c for c in cases if c[4] == it]
        chains = [c[1] for c in sub] + [c[2] for c in sub]
        n = len(sub)
        X = np.ascontiguousarray(np.concatenate(chains), np.float64)
        lens = np.array([len(c) for c in chains], np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
        pa, pb = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
        nl = np.array([_norm(c) for c in sub], np.int32)
        moff = np.concatenate([[0], np.cumsum(lens[:n], dtype=np.int64)[:-1]]).astype(np.int64)
        outs = []
        for ex in (False, True):
            tm, T, n_ali = np.full(n, -7.0), np.full((n, 12), -7.0), np.full(n, -7, np.int32)
            amap, stm = np.full(int(lens[:n].sum()), -7, np.int32), np.full((n, 5), -7.0)
            args = (0, P(X), P(offs), P(lens), 2 * n, P(pa), P(pb), P(nl), n, it, P(tm), P(T), P(n_ali), P(moff), P(amap))
            rc = lib.fd_tm_align_ex(*args, 3, P(stm)) if ex else lib.fd_tm_align(*args)
            assert rc == 0, lib.fd_last_error()
            outs.append((tm, T, n_ali, amap, stm))
        for old, new, what in zip(outs[0][:4], outs[1][:4], ("tm", "transform", "n_ali", "map")):
            assert old.tobytes() == new.tobytes(), (what, it)
        stm = outs[1][4]
        assert (stm[:, 2:] == -1).all() and np.array_equal(stm[:, :2].max(1), outs[1][0])


def test_all_starts_against_restatement(all_starts):
    """The all-starts parity set: |TM - restatement| <= 1e-9, equal maps, the per-start scores within 1e-9 and -1
    exactly where the restatement skips a start."""
    cases, want = ts.parity_set(), ts.parity_results()
    tm, _, _, maps, stm = all_starts
    dev = np.array([abs(tm[k] - want[k]["tm"]) for k in range(len(cases))])
    wrong = [k for k in range(len(cases)) if not np.array_equal(maps[k], want[k]["map"])]
    wstm = np.array([w["start_tms"] for w in want])
    sdev = np.abs(stm - wstm)
    _record("tmalign_starts_vs_restatement", max=dev.max(), per_start_max=sdev.max(), pairs=len(cases), maps_differ=len(wrong),
            min_margin=min(r["margin"] for r in want))
    assert not wrong, [(k, cases[k][0], len(cases[k][1]), len(cases[k][2])) for k in wrong]
    assert dev.max() <= 1e-9, [(k, cases[k][0], dev[k]) for k in np.flatnonzero(dev > 1e-9)]
    assert np.array_equal(stm == -1, wstm == -1)
    assert sdev.max() <= 1e-9, [(k, cases[k][0], sdev[k].tolist()) for k in np.flatnonzero(sdev.max(1) > 1e-9)]


def test_result_is_honest(all_starts):
    """TM recomputed in numpy from the returned R, t and map equals the returned TM within 1e-9; R is a proper
    rotation; the map is strictly increasing and within the second chain."""
    cases = ts.parity_set()
    tm, R, t, maps, _ = all_starts
    worst = 0.0
    for k, c in enumerate(cases):
        worst = max(worst, abs(ta.tm_of_map(c[1], c[2], R[k], t[k], maps[k], _norm(c)) - tm[k]))
        assert np.abs(R[k] @ R[k].T - np.eye(3)).max() < 1e-12 and np.linalg.det(R[k]) > 0
        m = maps[k][maps[k] >= 0]
        assert maps[k].shape == (len(c[1]),) and len(m) >= 1
        assert (np.diff(m) > 0).all() and m.max() < len(c[2]) and maps[k].min() >= -1
    _record("tmalign_starts_honest", max=worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("name", ["ss_dist", "local", "fragment"])
def test_single_start_against_restatement(gpu, name):
    """Each new start alone (bits 4, 8, 16) on three pairs -- a broken one, one where the new starts win, a short one
    (no start 4; this one has a break) -- matches the restatement with that selection, skipped starts included."""
    kinds = [c[0] for c in ts.parity_set()]
    sub = [ts.parity_set()[k] for k in (kinds.index("break_both"), kinds.index("core"), kinds.index("short") + 1)]
    tm, _, _, maps, stm = _align(sub, (name,))
    for k, c in enumerate(sub):
        want = ts.tm_align(c[1], c[2], Ln=c[3], max_iter=c[4], starts=(name,))
        assert want["margin"] >= 1e-9
        assert abs(tm[k] - want["tm"]) <= 1e-9 and np.array_equal(maps[k], want["map"]), (name, c[0], tm[k], want["tm"])
        assert np.array_equal(stm[k] == -1, want["start_tms"] == -1) and np.abs(stm[k] - want["start_tms"]).max() <= 1e-9


def test_more_starts_never_lower(all_starts, two_starts):
    """TM(31) >= TM(3) exactly for every pair, and where they are equal every output is identical; TM(3) through
    fd_tm_align_ex is what the default path (fd_tm_align) returns."""
    cases = ts.parity_set()
    default = structures.tm_align([c[1] for c in cases[:-1]], [c[2] for c in cases[:-1]], norm_lens=[_norm(c) for c in cases[:-1]])
    assert np.array_equal(default, two_starts[0][:-1])
    raised = 0
    for k in range(len(cases)):
        assert all_starts[0][k] >= two_starts[0][k], cases[k][0]
        assert np.array_equal(all_starts[4][k][:2], two_starts[4][k][:2])
        if all_starts[0][k] == two_starts[0][k]:
            assert all(np.array_equal(all_starts[q][k], two_starts[q][k]) for q in (1, 2, 3)), cases[k][0]
        else:
            raised += 1
    _record("tmalign_starts_raised", pairs=raised, of=len(cases), max_gain=(all_starts[0] - two_starts[0]).max())
    assert raised >= 3


def test_invariance(all_starts):
    """A rigid motion of either chain moves TM(31) by <= 1e-9."""
    cases = ts.parity_set()
    rng = np.random.default_rng(7)
    sub = list(range(0, len(cases) - 1, 2))
    moved_a = [cases[k][1] @ tr.rotation(rng).T + rng.uniform(-50, 50, 3) for k in sub]
    moved_b = [cases[k][2] @ tr.rotation(rng).T + rng.uniform(-50, 50, 3) for k in sub]
    nl = [_norm(cases[k]) for k in sub]
    worst = 0.0
    for A, B in ((moved_a, [cases[k][2] for k in sub]), ([cases[k][1] for k in sub], moved_b)):
        got = structures.tm_align(A, B, norm_lens=nl, starts="all")
        worst = max(worst, np.abs(got - all_starts[0][sub]).max())
    _record("tmalign_starts_invariance", max=worst)
    assert worst <= 1e-9


def test_batch_invariant(all_starts):
    """A pair aligned alone, and in a call of other pairs in another order, gives the bytes it gave in the full call."""
    cases = ts.parity_set()
    tm, R, t, maps, stm = all_starts
    for k in (1, 12, 20):
        one = _align([cases[k]], "all")
        assert one[0][0] == tm[k] and np.array_equal(one[1][0], R[k]) and np.array_equal(one[2][0], t[k])
        assert np.array_equal(one[3][0], maps[k]) and np.array_equal(one[4][0], stm[k])
    order = [20, 3, 12, 7, 1]
    some = _align([cases[k] for k in order], "all")
    for q, k in enumerate(order):
        assert some[0][q] == tm[k] and np.array_equal(some[3][q], maps[k]) and np.array_equal(some[4][q], stm[k])


def test_max_tm_across_refs_all_starts(gpu):
    """6 queries x 4 references: all starts >= the default element-wise, in the maxima and in every pair."""
    rng = np.random.default_rng(11)
    refs = [ts.core_pair(rng, 30, 20, 15, 10, 30)[0], tr.ca_chain(rng, 45), ts.broken(rng, tr.ca_chain(rng, 60), 2), tr.ca_chain(rng, 11)]
    queries = [tr.ca_chain(rng, int(n)) for n in (15, 40, 66)] + [ts.broken(rng, refs[1], 1), refs[0][25:70] + 0.2, refs[2][5:50]]
    best2, _ = structures.max_tm_across_refs(queries, refs)
    best5, which5 = structures.max_tm_across_refs(queries, refs, starts="all")
    assert (best5 >= best2).all() and which5.shape == (6,)
    pairs = [(i, 6 + j) for i in range(6) for j in range(4)]
    t2 = structures.pairwise_tm(queries + refs, pairs)
    t5 = structures.pairwise_tm(queries + refs, pairs, starts="all")
    _record("tmalign_starts_refs", raised=(t5 > t2).sum(), max_gain=(t5 - t2).max())
    assert (t5 >= t2).all() and np.array_equal(best5, t5.reshape(6, 4).max(1))

"""fp64 numpy restatement of the alignment search of ``fd_tm_align`` (DESIGN.md "TM-align-style alignment"), with the
decision margin of every run.

Deliberately a different route to the same definition: the search over aligned pairs is ``tm_reference.tm_search`` (SVD
fits), the labels are ``psea_reference.psea``, the dynamic programme fills whole anti-diagonals of full matrices, the
score matrix is built at once from all n1 x n2 distances through sqrt, and the threading fits are SVD fits in a plain
loop over the offsets.  Not collected by pytest (no ``test_`` prefix).

The definition (shared with the kernel's header comment and DESIGN.md):

* ``search(map)``: the TM-score search of ``tm_reference.tm_search`` over the aligned pairs (x_i, y_map[i]), normalised
  by Ln, at the smallest stride s >= 1 that leaves at most 256 seeds.
* ``DP(S, g)``: val[i][0] = val[0][j] = 0; D = val[i-1][j-1] + S[i-1][j-1], H = val[i-1][j] + (g if (i-1, j) was a
  match), V = val[i][j-1] + (g if (i, j-1) was a match); match if D >= H and D >= V, else up if H >= V, else left;
  trace back from (n1, n2) while i > 0 and j > 0, a match cell puts map[i-1] = j-1.
* start 1, gapless threading: offset k pairs x_i with y_{i-k}; every k whose overlap is >= max(m // 2, min(m, 5)),
  m = min(n1, n2), ascending; the score of k is the TM sum under the least-squares fit on its whole overlap; the largest
  wins, the first on a tie.
* start 2, secondary structure: S = 1 where the P-SEA labels are equal, else 0; DP(S, -1).
* refinement of a start map a0: search(a0) is a candidate; for g in (-0.6, 0.0), from search(a0)'s transform, up to
  max_iter times: S = 1 / (1 + |R x_i + t - y_j|^2 / d0^2), map = DP(S, g), stop if it equals the map of the iteration
  before (a0 at first), else search(map) is a candidate and gives the next transform.
* result: the candidate with the largest TM; the first wins a tie (start 1 before 2, g = -0.6 before 0, iterations in
  order)."""
import functools

import numpy as np

import psea_reference as pr
import tm_reference as tr

MAX_SEEDS = 256
GAP_OPENS = (-0.6, 0.0)
SS_GAP_OPEN = -1.0


def seed_count(n, stride):
    return len(tr.seeds(n, stride))


def search_stride(n_ali):
    """The smallest stride >= 1 at which an n_ali-residue search has at most MAX_SEEDS seeds."""
    s = 1
    while seed_count(n_ali, s) > MAX_SEEDS:
        s += 1
    return s


def aligned(x, y, amap):
    i = np.flatnonzero(amap >= 0)
    return x[i], y[amap[i]]


def search(x, y, amap, Ln):
    xa, ya = aligned(x, y, amap)
    return tr.tm_search(xa, ya, Ln=Ln, stride=search_stride(len(xa)))


def dp(S, g, exempt=False):
    """(map int [n1] with -1 for unaligned residues, the smallest best-minus-second-best over the cells of the traced
    path; inf when ``exempt``)."""
    n1, n2 = S.shape
    val = np.zeros((n1 + 1, n2 + 1))
    match = np.zeros((n1 + 1, n2 + 1), bool)
    choice = np.zeros((n1 + 1, n2 + 1), np.int8)   # 0 match, 1 up, 2 left
    gap = np.full((n1 + 1, n2 + 1), np.inf)
    for d in range(2, n1 + n2 + 1):
        i = np.arange(max(1, d - n2), min(n1, d - 1) + 1)
        j = d - i
        D = val[i - 1, j - 1] + S[i - 1, j - 1]
        H = val[i - 1, j] + np.where(match[i - 1, j], g, 0.0)
        V = val[i, j - 1] + np.where(match[i, j - 1], g, 0.0)
        m = (D >= H) & (D >= V)
        u = ~m & (H >= V)
        val[i, j] = np.where(m, D, np.where(u, H, V))
        match[i, j] = m
        choice[i, j] = np.where(m, 0, np.where(u, 1, 2))
        top = np.sort(np.stack([D, H, V]), axis=0)
        gap[i, j] = top[2] - top[1]
    amap = np.full(n1, -1, np.int64)
    margin = np.inf
    i, j = n1, n2
    while i > 0 and j > 0:
        margin = min(margin, gap[i, j])
        c = choice[i, j]
        if c == 0:
            amap[i - 1] = j - 1
            i, j = i - 1, j - 1
        elif c == 1:
            i -= 1
        else:
            j -= 1
    return amap, (np.inf if exempt else float(margin))


def threading_offsets(n1, n2):
    m = min(n1, n2)
    need = max(m // 2, min(m, 5))
    return [k for k in range(-(n2 - 1), n1) if min(n1, n2 + k) - max(0, k) >= need]


def threading(x, y, Ln):
    """(start map, best minus second-best offset score on the TM scale)."""
    n1, n2 = len(x), len(y)
    d0 = tr.d0(Ln)
    ks = threading_offsets(n1, n2)
    scores = []
    for k in ks:
        lo, hi = max(0, k), min(n1, n2 + k)
        xs, ys = x[lo:hi], y[lo - k:hi - k]
        R, t = tr.kabsch(xs, ys)
        d = np.sqrt(((xs @ R.T + t - ys) ** 2).sum(1))
        scores.append((1.0 / (1.0 + (d / d0) ** 2)).sum() / Ln)
    scores = np.array(scores)
    b = int(np.argmax(scores))
    k = ks[b]
    amap = np.full(n1, -1, np.int64)
    lo, hi = max(0, k), min(n1, n2 + k)
    amap[lo:hi] = np.arange(lo - k, hi - k)
    rest = np.delete(scores, b)
    return amap, (float(scores[b] - rest.max()) if rest.size else np.inf)


def ss_start(x, y):
    la = np.frombuffer(pr.psea(x).encode(), np.uint8)
    lb = np.frombuffer(pr.psea(y).encode(), np.uint8)
    S = (la[:, None] == lb[None, :]).astype(np.float64)
    return dp(S, SS_GAP_OPEN, exempt=True)[0]


def score_matrix(x, y, R, t, Ln):
    d = np.sqrt((((x @ R.T + t)[:, None, :] - y[None, :, :]) ** 2).sum(2))
    return 1.0 / (1.0 + (d / tr.d0(Ln)) ** 2)


def tm_align(x, y, Ln=None, max_iter=10, starts=("threading", "ss")):
    """dict(tm, R, t, map, n_ali, margin, candidates, start_tms) of the pair x [n1, 3], y [n2, 3].  ``map[i]`` is the
    residue of y aligned with residue i of x, or -1; y ~ x @ R.T + t.  ``start_tms``: the best TM reached from each
    start."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n1, n2 = len(x), len(y)
    Ln = n2 if Ln is None else int(Ln)
    assert n1 >= 1 and n2 >= 1 and Ln >= min(n1, n2) and max_iter >= 1
    margin = np.inf
    best = None          # (tm, R, t, map)
    n_cand = 0
    start_tms = []

    def offer(tm, R, t, amap):
        nonlocal best, margin, n_cand
        n_cand += 1
        if best is None:
            best = (tm, R, t, amap)
            return
        if not np.array_equal(amap, best[3]):
            margin = min(margin, abs(tm - best[0]))
        if tm > best[0]:
            best = (tm, R, t, amap)

    for start in starts:
        if start == "threading":
            a0, mg = threading(x, y, Ln)
            margin = min(margin, mg)
        else:
            a0 = ss_start(x, y)
        tm0, R0, t0 = search(x, y, a0, Ln)
        offer(tm0, R0, t0, a0)
        reached = tm0
        for g in GAP_OPENS:
            R, t, prev = R0, t0, a0
            for _ in range(max_iter):
                amap, mg = dp(score_matrix(x, y, R, t, Ln), g)
                margin = min(margin, mg)
                if np.array_equal(amap, prev):
                    break
                tm, R, t = search(x, y, amap, Ln)
                offer(tm, R, t, amap)
                reached = max(reached, tm)
                prev = amap
        start_tms.append(reached)
    tm, R, t, amap = best
    return dict(tm=tm, R=R, t=t, map=amap, n_ali=int((amap >= 0).sum()), margin=float(margin), candidates=n_cand,
                start_tms=start_tms)


def tm_of_map(x, y, R, t, amap, Ln):
    """TM(R, t) over the aligned pairs of ``amap``, normalised by Ln."""
    xa, ya = aligned(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(amap))
    return tr.tm_of(xa, ya, R, t, Ln=Ln)


# ---------------------------------------------------------------------------------------------------- test pairs
def _move(rng, a):
    return a @ tr.rotation(rng).T + rng.uniform(-40, 40, 3)


def deletion_pair(rng, n):
    """(a, b, the deleted residues): b = a without n // 10 consecutive residues, rotated and moved."""
    a = tr.ca_chain(rng, n)
    k = n // 10
    s = int(rng.integers(1, n - k))
    cut = np.arange(s, s + k)
    return a, _move(rng, np.delete(a, cut, axis=0)), cut


def insertion_pair(rng, n):
    """b = a with a loop of 3-8 residues inserted, 1 A noise, rotated and moved."""
    a = tr.ca_chain(rng, n)
    k = int(rng.integers(3, 9))
    s = int(rng.integers(2, n - 2))
    loop = a[s - 1] + tr.ca_chain(rng, k + 1)[1:]
    b = np.concatenate([a[:s], loop, a[s:] + (loop[-1] - a[s - 1])])
    return a, _move(rng, b + rng.standard_normal(b.shape))


def hinge_pair(rng, n, noise=0.0):
    """(a, b): b = a hinged at n // 2 (the second half rotated 90 degrees and moved 10 A) with n // 10 residues of the
    first half deleted, rotated and moved."""
    a = tr.ca_chain(rng, n)
    b = tr.two_domain(a, n // 2)
    k = max(1, n // 10)
    s = int(rng.integers(1, n // 2 - k))
    b = np.delete(b, np.arange(s, s + k), axis=0)
    return a, _move(rng, b + rng.standard_normal(b.shape) * noise)


def unrelated_pair(rng, n1, n2):
    return pr.segment_chain(rng, n1, 0.3), _move(rng, pr.segment_chain(rng, n2, 0.3))


@functools.lru_cache(maxsize=None)
def parity_set():
    """The seeded pairs of the parity tests: [(kind, a, b, Ln or None, max_iter)], 40 pairs of lengths 5-130 and one
    512 x 300 pair at max_iter = 2."""
    rng = np.random.default_rng(20240611)
    out = []
    sizes = [5, 8, 13, 21, 22, 34, 47, 64, 90, 130]
    for q, n in enumerate(sizes):
        a, b, _ = deletion_pair(rng, max(n, 10))
        out.append(("deletion", a, b, None, 10))
        a, b = insertion_pair(rng, n)
        out.append(("insertion", a, b, None if q % 2 else len(b) + 7, 10))
        a, b = hinge_pair(rng, max(n, 30), noise=0.5)
        out.append(("hinge", a, b, None, 10))
        a, b = unrelated_pair(rng, n, sizes[(q * 3 + 4) % len(sizes)])
        out.append(("unrelated", a, b, None, 10))
    a, b = unrelated_pair(rng, 512, 300)
    out.append(("unrelated", a, b, None, 2))
    return out


@functools.lru_cache(maxsize=None)
def parity_results():
    """``tm_align`` of every pair of ``parity_set()``, computed once per process and shared by the tests (read-only)."""
    return [tm_align(a, b, Ln=Ln, max_iter=it) for _, a, b, Ln, it in parity_set()]
